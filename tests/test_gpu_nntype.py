"""The nntype variants on the GPU, bitwise.

1. nngp_predict_listed on nngp_knn's own lists is nngp_predict_batch (preds, out, fits): every padded
   fit size at its edges, the finishing loop's four-coordinate trips (d = 63, 64, 65), D2 by waves
   (d = 129) and the (m, d) = (64, 95) / (64, 96) edge of the select's LDS staging; n_q = 1, 2, 5.
2. Arbitrary lists (reversed, permuted, one with a duplicated row) against the oracle's parts
   (nntype_ref.predict_listed).
3. nngp_listed_sweep against the per-slice loop (G launch, nngp_predict_listed with n_q = 1, update)
   in both forms: one wave (Lorenz: lane G; Burgers d = 64: wave G) and per-slice launches (FHN-PDE
   d_x = 4; Lorenz with the contracted G), N - I = 1, 2, 7; and FHN-PDE at d = 162 > 128, where the
   launch form takes kd2 from a launch of its own, N - I = 2.
4. run(model='nngp', nntype=t) for every listed t on the fixture's configuration against the CPU
   restated loop (nntype_ref.parareal over the oracle): K, conv_int and every iterate.  The restated
   loop's K is the reference's for all five types (checked on the CPU when this was written), so K
   is asserted against tests/golden/nntype.npz too; conv_int against the reference is printed (its
   Nelder-Mead fits stop at fatol = xatol = 0.1: DESIGN.md 3.3c).
5. run(model='nngp', nntype='row') is not run(model='nngp')."""
import ctypes
import functools

import numpy as np
import pytest

import knn_cases as KC
import nntype_ref as NR
import oracle as O
from conftest import golden

pytestmark = pytest.mark.gpu

JIT = np.arange(-20, -11, dtype=float)
SENT = -7.125e77   # what the output buffers hold before a call
ROWS, NQ = 80, 5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    """Equal as raw doubles, except that any NaN equals any NaN at the same position."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(_bits(np.nan_to_num(a, nan=7.0)), _bits(np.nan_to_num(b, nan=7.0)))


def _t(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device='cuda')


def _jp():
    return JIT.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _full(shape):
    import torch
    return torch.full(shape, SENT, dtype=torch.float64, device='cuda')


def draws(d, nq, seed=3):
    import nngp_amd
    return nngp_amd.NNGP_p(n=d, N=4, nn=10, seed=seed).draw_thetas(nq).reshape(nq, d * 9, 2)


def listed(gpu, X, Y, Q, lists, th0, bias=None):
    """nngp_predict_listed with every output: dict(preds, out, fits) on the host."""
    import torch
    rows, d = X.shape
    nq, m = lists.shape
    lists = np.ascontiguousarray(lists, dtype=np.int32)
    preds, fits = _full((nq, d)), _full((nq, d * 9, 4))
    bt = None if bias is None else _t(bias)
    out = None if bias is None else _full((nq, d))
    Xt, Yt, Qt, tht = _t(X), _t(Y), _t(Q), _t(th0)
    gpu._lib.check(gpu.lib().nngp_predict_listed(
        Xt.data_ptr(), Yt.data_ptr(), rows, d, Qt.data_ptr(), nq, lists.ctypes.data, m, 9, _jp(), 1, tht.data_ptr(),
        0.1, 0.1, 400, preds.data_ptr(), None if bt is None else bt.data_ptr(),
        None if out is None else out.data_ptr(), fits.data_ptr(), None))
    torch.cuda.synchronize()
    return dict(preds=preds.cpu().numpy(), out=None if out is None else out.cpu().numpy(), fits=fits.cpu().numpy())


# ------------------------------------------------------------------ 1. against nngp_predict_batch
SHAPES = ([(m, 3) for m in (1, 8, 9, 16, 17, 20, 24, 32, 33, 48, 64)] +
          [(20, d) for d in (1, 63, 64, 65, 129)] + [(64, 95), (64, 96)])


@functools.lru_cache(maxsize=None)
def knn_case(m, d):
    """(X, Y, Q [5][d], theta0, bias) and nngp_predict_batch's outputs for them, computed once."""
    import torch
    import nngp_amd as gpu
    X, Y, _ = KC.predict_data((m, d, ROWS))
    rng = np.random.default_rng(100 * m + d)
    Q = X[rng.choice(ROWS, size=NQ, replace=False)] + 0.01 * rng.standard_normal((NQ, d))
    th0, bias = draws(d, NQ), rng.standard_normal((NQ, d))
    preds, out, fits = _full((NQ, d)), _full((NQ, d)), _full((NQ, d * 9, 4))
    idx = torch.full((NQ, m), -7, dtype=torch.int32, device='cuda')
    Xt, Yt, Qt, tht, bt = _t(X), _t(Y), _t(Q), _t(th0), _t(bias)
    gpu._lib.check(gpu.lib().nngp_predict_batch(
        Xt.data_ptr(), Yt.data_ptr(), ROWS, d, Qt.data_ptr(), NQ, m, 9, _jp(), 1, tht.data_ptr(), 0.1, 0.1, 400,
        preds.data_ptr(), bt.data_ptr(), out.data_ptr(), idx.data_ptr(), fits.data_ptr(), None))
    torch.cuda.synchronize()
    ref = dict(preds=preds.cpu().numpy(), out=out.cpu().numpy(), fits=fits.cpu().numpy(), idx=idx.cpu().numpy())
    assert ref['idx'].min() >= 0 and not any(np.any(ref[k] == SENT) for k in ('preds', 'out', 'fits'))
    return X, Y, Q, th0, bias, ref


@pytest.mark.parametrize('nq', [1, 2, 5])
@pytest.mark.parametrize('m,d', SHAPES)
def test_listed_on_knn_lists_is_predict_batch(gpu, m, d, nq):
    X, Y, Q, th0, bias, ref = knn_case(m, d)
    got = listed(gpu, X, Y, Q[:nq], ref['idx'][:nq], th0[:nq], bias[:nq])
    for key in ('preds', 'out', 'fits'):
        assert _same(got[key], ref[key][:nq]), key


# ------------------------------------------------------------------------ 2. against the oracle
@pytest.mark.parametrize('m,d', [(8, 3), (20, 5)])
def test_arbitrary_lists_are_the_oracle_parts(gpu, m, d):
    X, Y, _ = KC.predict_data((m, d, ROWS))
    rng = np.random.default_rng(7 * m + d)
    Q = X[rng.choice(ROWS, size=4, replace=False)] + 0.01 * rng.standard_normal((4, d))
    knn = np.array([O.knn(X, q, m)[0] for q in Q])
    dup = rng.permutation(ROWS)[:m]
    if m > 1:
        dup[m - 1] = dup[0]
    lists = np.stack([knn[0][::-1], rng.permutation(knn[1]), rng.permutation(ROWS)[:m], dup]).astype(np.int32)
    th0 = draws(d, 4, seed=11)
    got = listed(gpu, X, Y, Q, lists, th0)
    for q in range(4):
        preds, fits = NR.predict_listed(X, Y, lists[q], Q[q], th0[q], return_fits=True)
        assert _same(got['fits'][q], fits), q
        assert _same(got['preds'][q], preds), q


# --------------------------------------------------------------------- 3. the sweep's two forms
def _system(gpu, name):
    if name == 'lorenz':
        return gpu.Lorenz(normalization='-11'), dict(Ng=6, G='RK4'), [0, 2.0]
    if name == 'lorenz_fma':
        return gpu.Lorenz(normalization='-11'), dict(Ng=6, G='RK4', fma=True), [0, 2.0]
    if name == 'burgers64':
        return gpu.Burgers(d_x=64, normalization='-11'), dict(Ng=4, G='RK4'), [0, 0.8]
    if name == 'fhnpde4':
        return gpu.FHN_PDE(d_x=4, normalization='-11'), dict(Ng=4, G='RK4'), [0, 0.8]
    return gpu.FHN_PDE(d_x=9, normalization='-11'), dict(Ng=4, G='RK2'), [0, 0.8]   # d = 162 > 128


SWEEPS = [(name, n_sl) for name in ('lorenz', 'burgers64', 'fhnpde4', 'lorenz_fma') for n_sl in (1, 2, 7)] + \
    [('fhnpde9', 2)]   # (1 458 fits per slice: two slices)


@pytest.mark.parametrize('name,n_sl', SWEEPS)
def test_listed_sweep_is_the_per_slice_loop(gpu, name, n_sl):
    import torch
    ode, skw, tspan = _system(gpu, name)
    s = gpu.SolverRK(ode.get_vector_field(), Nf=40, F='RK4', **skw)
    d, N, m, rows = ode.get_dim(), 8, 6, 40
    I = N - n_sl
    rng = np.random.default_rng(n_sl + 10 * d)
    u0 = np.asarray(ode.get_init_cond(), dtype=float)
    X = u0[None, :] + 0.05 * rng.standard_normal((rows, d))
    Y = 0.01 * np.sin(3 * X) + 1e-5 * rng.standard_normal((rows, d))
    lists = np.stack([rng.permutation(rows)[:m] for _ in range(n_sl)]).astype(np.int32)
    th0 = _t(draws(d, n_sl, seed=5))
    t_dev = _t(np.linspace(tspan[0], tspan[1], N + 1))
    Xt, Yt = _t(X), _t(Y)
    L, cs = gpu.lib(), s.f.csystem(Xt.device)

    def fresh():
        U1, UG1 = _full((N + 1, d)), _full((N + 1, d))
        U1[I] = _t(u0 + 0.01)
        return U1, UG1, _full((n_sl, d))

    # the per-slice loop: G launch, one listed prediction, the update (out = preds + bias)
    U1, UG1, P = fresh()
    for i in range(I, N):
        j = i - I
        s.run_G_batch(t_dev[i:i + 1], t_dev[i + 1:i + 2], U1[i:i + 1], out=UG1[i + 1:i + 2])
        gpu._lib.check(L.nngp_predict_listed(
            Xt.data_ptr(), Yt.data_ptr(), rows, d, U1[i].data_ptr(), 1, lists[j:j + 1].ctypes.data, m, 9, _jp(), 1,
            th0[j].data_ptr(), 0.1, 0.1, 400, P[j].data_ptr(), UG1[i + 1].data_ptr(), U1[i + 1].data_ptr(), None,
            None))
    torch.cuda.synchronize()
    want = [v.cpu().numpy() for v in (U1, UG1, P)]
    assert not np.any(want[0][I:] == SENT) and not np.any(want[1][I + 1:] == SENT) and not np.any(want[2] == SENT)

    U1, UG1, P = fresh()
    g_ms = ctypes.c_float(-1.0)
    gpu._lib.check(L.nngp_listed_sweep(
        ctypes.byref(cs), gpu._lib.TABLEAU[s.G], s.step_mode, s.Ng, t_dev.data_ptr(), I, N, U1.data_ptr(),
        UG1.data_ptr(), Xt.data_ptr(), Yt.data_ptr(), rows, lists.ctypes.data, m, 9, _jp(), 1, th0.data_ptr(), 0.1,
        0.1, 400, P.data_ptr(), ctypes.byref(g_ms), None))
    torch.cuda.synchronize()
    for got, w, what in zip((U1, UG1, P), want, ('U1', 'UG1', 'preds')):
        assert _same(got.cpu().numpy(), w), (name, what)
    assert g_ms.value >= 0.0


# ------------------------------------------------------------------------- 4. / 5. the driver
def _fixture_run(gpu, **kw):
    z = golden('nntype.npz')
    t0, t1, N, Ng, Nf, eps, nn = z['cfg']
    ode = gpu.Rossler(normalization='-11')
    s = gpu.SolverRK(ode.get_vector_field(), Ng=int(Ng), Nf=int(Nf), F='RK4', G='RK1')
    p = gpu.Parareal(ode, s, [t0, t1], int(N), epsilon=float(eps), verbose=None)
    return z, p.run(model='nngp', nn=int(nn), **kw)


@pytest.mark.parametrize('t', NR.LISTED)
def test_run_is_the_restated_loop(gpu, t):
    z, r = _fixture_run(gpu, nntype=t)
    t0, t1, N, Ng, Nf, eps, nn = z['cfg']
    o = NR.parareal(O.System('rossler'), [t0, t1], int(N), int(Ng), int(Nf), 'RK1', 'RK4', t, int(nn), epsilon=eps,
                    u0=z['u0'])
    print(f"{t}: K gpu {r['k']} restated {o['k']} reference {int(z[f'{t}__k'])}; conv_int gpu {r['conv_int']} "
          f"reference {z[f'{t}__conv_int'].tolist()}")
    assert r['k'] == o['k'] and r['conv_int'] == o['conv_int'] and r['converged'] == o['converged']
    assert np.array_equal(np.nan_to_num(r['u'], nan=7.0), np.nan_to_num(o['u'], nan=7.0))
    assert r['k'] == int(z[f'{t}__k'])   # the reference's K (the restated loop reproduces it for every type)


def test_debug_and_comparison_paths_predict_on_the_lists(gpu):
    """debug=True sweeps slice by slice through predict_device (one nngp_predict_listed query), and a
    listed model among comp_mdls predicts all slices in one call: the same iterates as the sweep."""
    z, r = _fixture_run(gpu, nntype='col_full')
    _, rd = _fixture_run(gpu, nntype='col_full', debug=True,
                         comp_mdls=[gpu.NNGP_alt(n=3, N=10, nntype='row_col', nn=int(z['cfg'][6]))])
    assert rd['k'] == r['k'] and rd['conv_int'] == r['conv_int']
    assert np.array_equal(np.nan_to_num(rd['u'], nan=7.0), np.nan_to_num(r['u'], nan=7.0))
    errs = rd['err_store_mdls']['NNGProw_col']
    assert len(errs[0]) == 9 and not np.any(np.isnan(errs[0]))   # iteration 0: slices 1 .. 9


def test_nntype_row_is_not_plain_nngp(gpu):
    _, plain = _fixture_run(gpu)
    _, row = _fixture_run(gpu, nntype='row')
    assert np.array_equal(plain['u'][:, :, 0], row['u'][:, :, 0])   # the initial coarse sweep
    K = min(plain['u'].shape[2], row['u'].shape[2])
    assert K >= 2 and not np.array_equal(plain['u'][:, :, 1:K], row['u'][:, :, 1:K])
    _, nn = _fixture_run(gpu, nntype='nn')   # 'nn' is the parent's path
    assert nn['k'] == plain['k'] and np.array_equal(np.nan_to_num(nn['u'], nan=7.0), np.nan_to_num(plain['u'], nan=7.0))
