"""GPU: the ELM kernels, entry points and driver against the NumPy restatement of the arithmetic
contract (tests/elm_ref.py), bit for bit.  The restatement itself is checked on the
CPU against the reference's ELM_base (tests/test_elm_host.py)."""
import numpy as np
import pytest

import elm_ref as E
from conftest import golden
from systems_table import burgers_u0, oracle_burgers, product_burgers
from elm_cases import EPS, RUNS, cpu_loop, serial_fine

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    a, b = np.nan_to_num(a, nan=7.0), np.nan_to_num(b, nan=7.0)   # columns not written stay NaN
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


# ------------------------------------------------------------------------------ nngp_elm_hidden
# n_poly = 6 and 10 (below a wave), 78 (just past 64 lanes), 8 385 and 20 301 (several chunks); 4 at degree 1
@pytest.mark.parametrize('d,deg', [(2, 2), (3, 2), (11, 2), (128, 2), (200, 2), (3, 1)])
def test_hidden_rows_are_bitwise_the_restatement(gpu, d, deg):
    rng = np.random.default_rng(100 + d)
    X = rng.uniform(-1, 1, (70, d))
    Xd = _dev(X)
    for res in (1, 20, 50):
        mdl = gpu.ELM_base(d=d, res_size=res, degree=deg)
        bias, C = E.draw_weights(d, 47, res, deg)
        ref = E.hidden(X, bias, C, deg)
        assert np.any(ref > 0)
        for rows in (1, 5, 70):
            got = mdl.hidden_device(Xd[:rows]).cpu().numpy()
            assert np.array_equal(_bits(got), _bits(ref[:rows])), (res, rows)
        two = np.vstack([mdl.hidden_device(Xd[:3]).cpu().numpy(), mdl.hidden_device(Xd[3:]).cpu().numpy()])
        assert np.array_equal(_bits(two), _bits(ref)), res


# ----------------------------------------------------------------------------- nngp_elm_predict
def _ref_predict(X, Y, q, m, bias, C, deg=2):
    idx = E.knn(X, q, m)
    return E.solve(E.hidden(X[idx], bias, C, deg), Y[idx], E.hidden(q, bias, C, deg)[0])


def _gpu_predict(mdl, X, Y, q, ug=None):
    """(preds, preds + ug) through ELM_base's device path, from a training set given as host arrays."""
    import torch
    mdl.fit(X, Y, 0)
    qd = _dev(q)
    if ug is None:
        return mdl.predict_device(qd).cpu().numpy(), None
    out, preds = torch.empty_like(qd), torch.empty_like(qd)
    mdl.predict_device(qd, out=out, bias=_dev(ug), preds=preds)
    only = torch.empty_like(qd)
    mdl.predict_device(qd, out=only, bias=_dev(ug))   # without the bare prediction
    assert np.array_equal(_bits(only.cpu().numpy()), _bits(out.cpu().numpy()))
    return preds.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize('d', [3, 128])
@pytest.mark.parametrize('m', [1, 2, 4, 7, 16])
def test_predictions_are_bitwise_the_restatement(gpu, d, m):
    rng = np.random.default_rng(7 * d + m)
    bias, C = E.draw_weights(d, 47, 20, 2)
    Xall, Yall = rng.uniform(-1, 1, (5000, d)), rng.uniform(-1, 1, (5000, d))
    q, ug = rng.uniform(-1, 1, d), rng.uniform(-1, 1, d)
    for rows in (m, 40, 5000):
        X, Y = Xall[:rows], Yall[:rows]
        ref = _ref_predict(X, Y, q, m, bias, C)
        assert np.all(np.isfinite(ref))
        mdl = gpu.ELM_base(d=d, res_size=20, m=m)
        preds, out = _gpu_predict(mdl, X, Y, q, ug)
        assert np.array_equal(_bits(preds), _bits(ref)), rows
        assert np.array_equal(_bits(out), _bits(ref + ug)), rows
        bare, _ = _gpu_predict(mdl, X, Y, q)
        assert np.array_equal(_bits(bare), _bits(ref)), rows
        assert np.array_equal(_bits(mdl.predict(q[None, :])), _bits(ref))   # the reference's host signature


def test_duplicated_neighbours_and_distance_ties(gpu):
    rng = np.random.default_rng(11)
    d = 3
    bias, C = E.draw_weights(d, 47, 20, 2)
    # the nearest neighbour twice (Parareal training sets hold converged states again and again)
    X = rng.uniform(-1, 1, (30, d))
    Y = rng.uniform(-1, 1, (30, d))
    q = X[4] + 1e-3
    X2, Y2 = np.vstack([X, X[4:5], X[9:10]]), np.vstack([Y, Y[4:5], Y[9:10]])
    for m in (2, 4, 7):
        ref = _ref_predict(X2, Y2, q, m, bias, C)
        got, _ = _gpu_predict(gpu.ELM_base(d=d, res_size=20, m=m), X2, Y2, q)
        assert np.all(np.isfinite(got)) and np.array_equal(_bits(got), _bits(ref)), m
    less = _ref_predict(X, Y, q, 3, bias, C)   # m = 4 with the duplicate = m = 3 without it
    got, _ = _gpu_predict(gpu.ELM_base(d=d, res_size=20, m=4), X2, Y2, q)
    assert np.array_equal(_bits(got), _bits(less))
    # ties in distance: the lattice {-1/2, 0, 1/2}^3 around q = 0 (6 rows at 1/4, 12 at 1/2): (distance, row) order
    g = np.array([-0.5, 0.0, 0.5])
    L = np.array([[a, b, c] for a in g for b in g for c in g])
    YL = rng.uniform(-1, 1, L.shape)
    for m in (4, 7, 16):
        ref = _ref_predict(L, YL, np.zeros(d), m, bias, C)
        got, _ = _gpu_predict(gpu.ELM_base(d=d, res_size=20, m=m), L, YL, np.zeros(d))
        assert np.array_equal(_bits(got), _bits(ref)), m


# ----------------------------------------------------------------- the sweep and the whole runs
def _lorenz(gpu, N=32):
    ode = gpu.Lorenz(normalization='-11')
    s = gpu.SolverRK(ode.get_vector_field(), Ng=6, Nf=450, F='RK4', G='RK4')
    return ode, s, gpu.Parareal(ode, s, [0, 18], N, epsilon=EPS, verbose=None)


def _fhn(gpu):
    ode = gpu.FHN_ODE(normalization='-11')
    s = gpu.SolverRK(ode.get_vector_field(), Ng=4, Nf=400, F='RK4', G='RK2')
    return ode, s, gpu.Parareal(ode, s, [0, 40], 40, epsilon=EPS, verbose=None)


_runs = {}


def gpu_run(gpu, name):
    """The GPU's whole run, computed once per session and left unchanged."""
    if name not in _runs:
        r = {'lorenz': _lorenz, 'fhn_ode': _fhn}[name](gpu)[2].run(model='elm', add_model=True)
        r['u'].setflags(write=False)
        _runs[name] = r
    return _runs[name]


def test_native_sweep_equals_the_per_slice_paths_and_the_restatement(gpu, monkeypatch):
    o = cpu_loop('lorenz')
    ode, s, p = _lorenz(gpu)
    native = p.run(model='elm', early_stop=4)
    assert native['k'] == 4 and _same(native['u'], o['u'][:, :, :4])
    dbg = _lorenz(gpu)[2].run(model='elm', early_stop=4, debug=True)
    assert _same(dbg['u'], native['u']) and len(dbg['debug_dict']['all_pred_err']) == 4
    ode2, s2, p2 = _lorenz(gpu)
    monkeypatch.setattr(s2, 'coarse_is_paged', lambda: True)   # the driver's per-slice Python sweep
    per_slice = p2.run(model='elm', early_stop=4)
    assert _same(per_slice['u'], native['u']) and per_slice['conv_int'] == native['conv_int']


@pytest.mark.parametrize('name', sorted(RUNS))
def test_whole_run_is_bitwise_the_restatement_loop(gpu, name):
    o, r = cpu_loop(name), gpu_run(gpu, name)
    assert r['k'] == o['k'] and r['conv_int'] == o['conv_int'] and r['converged']
    assert _same(r['u'], o['u']) and _same(r['err'], o['err'])
    assert np.array_equal(r['x'], o['x']) and np.array_equal(_bits(r['D']), _bits(o['D']))
    tm = r['timings']
    for key in ('mdl_train_t', 'mdl_pred_t', 'mdl_tot_t', 'by_iter', 'F_time', 'G_time', 'runtime'):
        assert key in tm
    assert tm['mdl_pred_t'] > 0 and tm['mdl_tot_t'] >= tm['mdl_pred_t']
    mdl = r['mdl']   # add_model=True: mdl.store(), host arrays only: the training set of its last fit
    rows = mdl.x.shape[0]   # (a run that ends by exhausting its slices appends one row it never fits)
    assert mdl.name == 'ELM' and mdl.ELM._dev is None and rows >= o['x'].shape[0] - 1
    assert np.array_equal(mdl.x, o['x'][:rows]) and np.array_equal(_bits(mdl.y), _bits(o['D'][:rows]))


@pytest.mark.parametrize('name', sorted(RUNS))
def test_run_converges_no_later_than_classic_parareal(gpu, name):
    z = golden('elm.npz')
    r = gpu_run(gpu, name)
    assert r['converged'] and r['k'] <= int(z[f'run__{name}__parareal__k'])


@pytest.mark.parametrize('name', sorted(RUNS))
def test_run_final_state_is_within_10_eps_of_the_serial_fine_solution(gpu, name):
    """The convergence condition on the GPU; the figures are those of
    test_elm_host.test_loop_final_state_is_within_10_eps_of_the_serial_fine_solution (the runs are
    bitwise the CPU loop's): Lorenz 4.64e-6, FHN-ODE 4.49e-9."""
    r = gpu_run(gpu, name)
    e = np.max(np.abs(r['u'][:, :, -1] - serial_fine(name)))
    print(f'{name}: final state is {e:.3e} from the serial fine solution (10 eps = {10 * EPS:.1e})')
    assert e <= 10 * EPS, e


def test_burgers_d64_short_schedule_is_bitwise_the_restatement_loop(gpu):
    d, N = 64, 16
    so = oracle_burgers(d, True)
    o = E.parareal_elm(so, [0, 0.625], N, 8, 400, 'RK2', 'RK4', epsilon=1e-13, u0=so.fit(burgers_u0(d)), early_stop=3)
    assert o['conv_int'] == [1, 2, 3] and np.all(np.isfinite(o['u']))   # three full sweeps, on the restatement
    ode = product_burgers(gpu, d, True)
    s = gpu.SolverRK(ode.get_vector_field(), Ng=8, Nf=400, F='RK4', G='RK2')
    r = gpu.Parareal(ode, s, [0, 0.625], N, epsilon=1e-13, verbose=None).run(model='elm', early_stop=3)
    assert r['k'] == 3 and r['conv_int'] == o['conv_int'] and _same(r['u'], o['u']) and _same(r['err'], o['err'])


def test_light_driver_and_checkpoint_resume(gpu, tmp_path):
    full = gpu_run(gpu, 'fhn_ode')
    ode, s, p = _fhn(gpu)
    light = gpu.PararealLight(ode, s, [0, 40], 40, epsilon=EPS, verbose=None).run(model='elm', early_stop=3)
    assert light['u'].shape == (41, 2) and _same(light['u'], full['u'][:, :, 3])
    assert light['conv_int'] == full['conv_int'][:3]
    again = p.run(model='elm', store_int=True, int_dir=str(tmp_path), int_name='fh')
    assert _same(again['u'], full['u'])
    p2 = _fhn(gpu)[2]
    res = p2.load_int_dump(str(tmp_path / 'fh' / 'fh_2.npz'))
    assert res['k'] == full['k'] and res['conv_int'] == full['conv_int']
    assert _same(res['u'], full['u']) and _same(res['err'], full['err'])
    assert np.array_equal(res['x'], full['x']) and np.array_equal(res['D'], full['D'])
