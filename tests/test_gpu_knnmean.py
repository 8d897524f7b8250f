"""GPU: the k-NN mean kernels, entry points, the models.NN driver paths and the Figure 2 model
comparison (comp_mdls) against the NumPy restatement of the contract (tests/knnmean_ref.py,
DESIGN.md §3.7), bit for bit.  The restatement itself is checked on the CPU against the reference's
NN model and comparison loop (tests/test_knnmean_host.py)."""
import numpy as np
import pytest

import knn_cases as KC
import knnmean_ref as KR
import oracle as O
from conftest import golden

pytestmark = pytest.mark.gpu

EPS = 5e-7
COMP_NN = KR.COMP_NN
SIXTEEN = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 30, 31, 33, 63, 64]
MIXED = [10, 1, 30, 4, 1]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    a, b = np.nan_to_num(a, nan=7.0), np.nan_to_num(b, nan=7.0)   # columns not written stay NaN
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(a, offset=False):
    """Device copy; offset: the array starts one double into its buffer (8-byte aligned only)."""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not offset:
        return torch.tensor(a, device='cuda')
    buf = torch.empty(a.size + 1, dtype=torch.float64, device='cuda')
    buf[1:] = torch.tensor(a.reshape(-1), device='cuda')
    return buf[1:].view(a.shape)


def gpu_means(gpu, X, Y, Q, counts, want_idx=False, offset=False):
    """nngp_knn_mean through models.NN: [len(counts)][n_q][d] (and idx [n_q][max count])."""
    import torch
    mdl = gpu.NN(N=4, nn=max(counts))
    mdl.fit(_dev(X, offset), _dev(Y), 0)
    Qd = _dev(np.atleast_2d(Q), offset)
    idx = torch.full((Qd.shape[0], max(counts)), -1, dtype=torch.int32, device='cuda') if want_idx else None
    out = mdl.predict_batch_device(Qd, counts=counts, idx_out=idx).cpu().numpy()
    return (out, idx.cpu().numpy()) if want_idx else out


def ref_means(X, Y, Q, counts, want_idx=False):
    both = [KR.knn_mean(X, Y, q, counts, return_idx=True) for q in np.atleast_2d(Q)]
    out = np.stack([b[0] for b in both], axis=1)
    return (out, np.stack([b[1] for b in both])) if want_idx else out


def _data(rows, d, n_q, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((rows, d))
    Y = 0.01 * np.sin(3 * X) + 1e-4 * rng.standard_normal((rows, d))
    Q = X[rng.integers(0, rows, n_q)] + 1e-2 * rng.standard_normal((n_q, d))
    return X, Y, Q


# --------------------------------------------------------------------------------- the kernels
# one select instantiation each (K = 2, 4, 8, 16 up to 4096 rows, streaming above) and the LDS key cache's edge
# from both sides: 14 336 rows is the kernel's largest dynamic LDS (112 KB of keys beside 20 KB static)
@pytest.mark.parametrize('rows', [1, 257, 513, 1025, 2049, 4097, 14336, 14337])
def test_every_select_form_feeds_the_mean_bitwise(gpu, rows):
    X, Y, Q = _data(rows, 3, 511, 100 + rows)
    clamp = lambda cs: [min(c, rows) for c in cs]
    lists = [[1], clamp([64]), clamp(MIXED)] + ([[rows]] if rows <= 64 else [])
    for n_q, cl in [(1, lists), (3, lists), (511, [clamp(SIXTEEN)])]:
        for counts in cl:
            got, idx = gpu_means(gpu, X, Y, Q[:n_q], counts, want_idx=True)
            ref, ref_idx = ref_means(X, Y, Q[:n_q], counts, want_idx=True)
            assert got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref)), (n_q, counts)
            assert np.array_equal(idx, ref_idx), (n_q, counts)


# the coordinate loop's tails are at 256 (thread c owns c, c + 256, ..)
@pytest.mark.parametrize('d', [1, 2, 33, 255, 256, 257, 800])
def test_every_coordinate_tail_bitwise(gpu, d):
    X, Y, Q = _data(300, d, 511, 200 + d)
    for n_q, cl in [(1, [[1], [64]]), (3, [MIXED, SIXTEEN]), (511, [MIXED])]:
        for counts in cl:
            got = gpu_means(gpu, X, Y, Q[:n_q], counts)
            assert np.array_equal(_bits(got), _bits(ref_means(X, Y, Q[:n_q], counts))), (n_q, counts)


def test_idx_out_is_nngp_knns_list(gpu):
    import torch
    X, Y, Q = _data(5000, 8, 6, 7)
    _, idx = gpu_means(gpu, X, Y, Q, [18, 5], want_idx=True)
    Xd = _dev(X)
    one = torch.empty(18, dtype=torch.int32, device='cuda')
    for j, q in enumerate(Q):
        gpu._lib.check(gpu.lib().nngp_knn(Xd.data_ptr(), 5000, 8, _dev(q).data_ptr(), 18, one.data_ptr(), None,
                                          torch.cuda.current_stream().cuda_stream))
        assert np.array_equal(one.cpu().numpy(), idx[j]), j


def test_ties_go_through_the_round_fallback(gpu):
    """300 copies of one row (knn_cases' tie case): more candidates than the threshold select ranks,
    so the m-round fallback feeds the mean, in (distance, row) order = row order."""
    case = next(c for c in KC.CASES if c['id'] == 'tie-r300-L300-m64')
    X, q = KC.build(case)
    assert KC.n_candidates(KC.ref_knn(X, q, 64)[2], 64) > KC.SEL_CAND
    Y = np.random.default_rng(5).standard_normal(X.shape)
    got, idx = gpu_means(gpu, X, Y, q, [64, 1, 33], want_idx=True)
    assert np.array_equal(idx[0], np.arange(64))
    assert np.array_equal(_bits(got), _bits(ref_means(X, Y, q, [64, 1, 33])))


def test_nan_and_inf_rows_propagate(gpu):
    X, Y, Q = _data(300, 5, 3, 11)
    for q in Q:   # the third and sixth nearest rows of every query
        i = KR.knn_mean_idx(X, q, 6)
        Y[i[2], 1] = np.nan
        Y[i[5]] = np.inf
    got = gpu_means(gpu, X, Y, Q, [2, 3, 5, 6, 30])
    ref = ref_means(X, Y, Q, [2, 3, 5, 6, 30])
    assert np.isfinite(ref[0]).all() and np.isnan(ref[1][:, 1]).all() and np.isinf(ref[3][:, 0]).all()
    assert np.array_equal(_bits(got), _bits(ref))


def test_batch_and_count_independence(gpu):
    X, Y, Q = _data(1500, 3, 511, 13)
    batch = gpu_means(gpu, X, Y, Q, [1, 2, 4, 10])
    alone = gpu_means(gpu, X, Y, Q[200], [1, 2, 4, 10])
    assert np.array_equal(_bits(batch[:, 200]), _bits(alone[:, 0]))
    four = gpu_means(gpu, X, Y, Q, [4])
    assert np.array_equal(_bits(batch[2]), _bits(four[0]))


def test_device_arguments_are_checked_before_they_are_read_by_address(gpu):
    import torch
    X, Y, Q = _data(40, 4, 6, 3)
    mdl = gpu.NN(N=4, nn=3)
    mdl.fit(_dev(X), _dev(Y), 0)
    Qd = _dev(Q)
    good = mdl.predict_batch_device(Qd).cpu().numpy()
    assert np.array_equal(_bits(good), _bits(ref_means(X, Y, Q, [3])))
    wide = _dev(np.hstack([Q, Q]))
    for bad, word in [(wide[:, :4], 'not contiguous'), (Qd.float(), 'float32'), (Qd[:, :3], 'shape'),
                      (Qd.cpu(), 'cpu'), (Q, 'device tensor')]:
        with pytest.raises(ValueError, match=word):
            mdl.predict_batch_device(bad)
    with pytest.raises(ValueError, match='out'):
        mdl.predict_batch_device(Qd, out=torch.empty((1, 6, 5), dtype=torch.float64, device='cuda'))
    with pytest.raises(ValueError, match='idx_out'):
        mdl.predict_batch_device(Qd, idx_out=torch.empty((6, 3), dtype=torch.int64, device='cuda'))
    with pytest.raises(ValueError, match='new_x'):
        mdl.predict_device(Qd[0].float())
    with pytest.raises(ValueError, match='preds'):
        mdl.predict_device(Qd[0], preds=wide[0, ::2])
    strided = gpu.NN(N=4, nn=3)
    strided.fit(_dev(np.hstack([X, X]))[:, :4], _dev(Y), 0)
    with pytest.raises(ValueError, match='x must be'):
        strided.predict_batch_device(Qd)


@pytest.mark.parametrize('d', [3, 33, 64])
def test_single_query_bias_and_unaligned_buffers(gpu, d):
    import torch
    X, Y, Q = _data(300, d, 1, 17 + d)
    ug = np.random.default_rng(d).standard_normal(d)
    ref = KR.knn_mean(X, Y, Q[0], [15])[0]
    for offset in (False, True):
        mdl = gpu.NN(N=4, nn=15)
        mdl.fit(_dev(X, offset), _dev(Y), 0)
        q = _dev(Q[0], offset)
        out, preds = torch.empty(d, dtype=torch.float64, device='cuda'), torch.empty(d, dtype=torch.float64, device='cuda')
        ret = mdl.predict_device(q, out=out, bias=_dev(ug), preds=preds)
        assert ret is preds and np.array_equal(_bits(preds.cpu().numpy()), _bits(ref)), offset
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(ref + ug)), offset
        assert np.array_equal(_bits(mdl.predict_device(q).cpu().numpy()), _bits(ref))
    host = gpu.NN(N=4, nn=15)
    host.fit(X, Y, 0)                                       # the reference's host signature
    assert np.array_equal(_bits(host.predict(Q[0][None, :], None, None, i=0)), _bits(ref))
    few = gpu.NN(N=4, nn=15)
    few.fit(X[:5], Y[:5], 0)                                # fewer rows than nn: all of them
    assert np.array_equal(_bits(few.predict(Q[0][None, :])), _bits(KR.knn_mean(X[:5], Y[:5], Q[0], [5])[0]))


# ---------------------------------------------------------------------------------- the driver
def _lorenz(gpu, cls=None, N=32):
    ode = gpu.Lorenz(normalization='-11')
    s = gpu.SolverRK(ode.get_vector_field(), Ng=6, Nf=450, F='RK4', G='RK4')
    return ode, (cls or gpu.Parareal)(ode, s, [0, 18], N, epsilon=EPS, verbose=None)


def _lorenz_ref(**kw):
    so = O.System('lorenz')
    return KR.parareal_compare(so, [0, 18], 32, 6, 450, 'RK4', 'RK4', epsilon=EPS, u0=so.fit([-15, -15, 20]), **kw)


_cache = {}


def cached(key, make):
    """A run computed once per session, shared by the tests that need it and left unchanged."""
    if key not in _cache:
        r = make()
        r['u'].setflags(write=False)
        _cache[key] = r
    return _cache[key]


def lorenz_nn_ref():
    return cached('lorenz_nn_ref', lambda: _lorenz_ref(model='nn', nn=3, early_stop=4))


def lorenz_nn_run(gpu):
    return cached('lorenz_nn_gpu', lambda: _lorenz(gpu)[1].run(model='nn', nn=3, early_stop=4, add_model=True))


def _check_run(r, o):
    assert r['k'] == o['k'] and r['conv_int'] == o['conv_int']
    assert _same(r['u'], o['u']) and _same(r['err'], o['err'])
    assert np.array_equal(r['x'], o['x']) and np.array_equal(_bits(r['D']), _bits(o['D']))


def test_lorenz_run_is_bitwise_the_restated_loop(gpu):
    """The lane form of G."""
    r, o = lorenz_nn_run(gpu), lorenz_nn_ref()
    assert r['k'] == 4 and 'err_store_mdls' not in r
    _check_run(r, o)
    mdl = r['mdl']
    assert mdl.name == '3-NN' and mdl._dev_xy is None and np.array_equal(mdl.x, o['x'][:mdl.x.shape[0]])
    assert r['timings']['mdl_pred_t'] > 0


def test_fhn_pde_run_is_bitwise_the_restated_loop(gpu):
    """d = 32, the field form of G."""
    ode = gpu.FHN_PDE(d_x=4)
    s = gpu.SolverRK(ode.get_vector_field(), Ng=10, Nf=100, F='RK8', G='RK4')
    r = gpu.Parareal(ode, s, [0, 4], 8, epsilon=1e-13, verbose=None).run(model='nn', nn=3, early_stop=3)
    so = O.System('fhn_pde', nx=4, normalized=False)
    o = KR.parareal_compare(so, [0, 4], 8, 10, 100, 'RK4', 'RK8', epsilon=1e-13, u0=ode.get_init_cond(), model='nn',
                            nn=3, early_stop=3)
    assert np.all(np.isfinite(o['u'])) and o['k'] == 3
    _check_run(r, o)


def test_burgers_run_is_bitwise_the_restated_loop(gpu):
    """d = 16, Burgers' form of G."""
    ode = gpu.Burgers(d_x=16, normalization='-11')
    s = gpu.SolverRK(ode.get_vector_field(), Ng=10, Nf=100, F='RK4', G='RK1')
    r = gpu.Parareal(ode, s, [0, 1], 8, epsilon=1e-13, verbose=None).run(model='nn', nn=3, early_stop=3)
    so = O.System('burgers', d=16, param=(0.01,), mn=0, mx=1)
    o = KR.parareal_compare(so, [0, 1], 8, 10, 100, 'RK1', 'RK4', epsilon=1e-13, u0=ode.get_init_cond(), model='nn',
                            nn=3, early_stop=3)
    assert np.all(np.isfinite(o['u'])) and o['k'] == 3
    _check_run(r, o)


# The sweep's launch computes its query's distances itself, a workgroup per 64 rows, and the workgroup that
# finishes last runs the select and the mean: several workgroups with a tail (300, 700 rows), the streaming
# select with its LDS key cache behind them (5000 rows, and 14 336: the largest cache, which every workgroup
# of this grid allocates), d = 3 and 18.  The runs above stay below 256 rows.
@pytest.mark.parametrize('system,rows', [('lorenz', 300), ('lorenz', 5000), ('lorenz', 14336), ('fhn18', 700)])
def test_native_sweep_on_a_large_training_set(gpu, system, rows):
    import ctypes
    import torch
    if system == 'lorenz':
        ode, so = gpu.Lorenz(normalization='-11'), O.System('lorenz')
        s = gpu.SolverRK(ode.get_vector_field(), Ng=6, Nf=45, F='RK4', G='RK4')
        order, Ng, T = 4, 6, 4.5
    else:
        ode, so = gpu.FHN_PDE(d_x=3), O.System('fhn_pde', nx=3, normalized=False)
        s = gpu.SolverRK(ode.get_vector_field(), Ng=10, Nf=100, F='RK8', G='RK4')
        order, Ng, T = 4, 10, 4.0
    N, I, m, d = 8, 2, 7, ode.get_dim()
    t = np.linspace(0, T, N + 1)
    rng = np.random.default_rng(rows + d)
    u0 = np.asarray(ode.get_init_cond(), dtype=np.float64)
    X = u0 + 0.05 * rng.standard_normal((rows, d))
    Y = 1e-3 * rng.standard_normal((rows, d))
    U1 = np.zeros((N + 1, d))
    UG1 = np.zeros((N + 1, d))
    U1[I] = u0
    ref_p = np.zeros((N - I, d))
    for i in range(I, N):
        UG1[i + 1] = so.rk(order, t[i], t[i + 1], Ng, U1[i])
        ref_p[i - I] = KR.knn_mean(X, Y, U1[i], [m])[0]
        U1[i + 1] = ref_p[i - I] + UG1[i + 1]
    assert np.all(np.isfinite(U1))
    U1d, UG1d = _dev(np.where(np.arange(N + 1)[:, None] <= I, U1, 0.0)), _dev(np.zeros((N + 1, d)))
    P = torch.zeros((N - I, d), dtype=torch.float64, device='cuda')
    Xd, Yd, td = _dev(X), _dev(Y), _dev(t)
    cs = s.f.csystem(U1d.device)
    g_ms = ctypes.c_float(-1.0)
    gpu._lib.check(gpu.lib().nngp_knn_mean_sweep(
        ctypes.byref(cs), gpu._lib.TABLEAU['RK4'], s.step_mode, Ng, td.data_ptr(), I, N, U1d.data_ptr(),
        UG1d.data_ptr(), Xd.data_ptr(), Yd.data_ptr(), rows, m, P.data_ptr(), ctypes.byref(g_ms),
        torch.cuda.current_stream().cuda_stream))
    assert np.array_equal(_bits(P.cpu().numpy()), _bits(ref_p))
    assert np.array_equal(_bits(U1d.cpu().numpy()[I:]), _bits(U1[I:]))
    assert np.array_equal(_bits(UG1d.cpu().numpy()[I + 1:]), _bits(UG1[I + 1:])) and g_ms.value > 0


def test_debug_and_per_slice_paths_leave_the_run_unchanged(gpu, monkeypatch):
    native = lorenz_nn_run(gpu)
    dbg = _lorenz(gpu)[1].run(model='nn', nn=3, early_stop=4, debug=True)
    assert _same(dbg['u'], native['u']) and dbg['conv_int'] == native['conv_int']
    assert len(dbg['debug_dict']['all_pred_err']) == 4 and 'err_store_mdls' not in dbg
    ode, p = _lorenz(gpu)
    monkeypatch.setattr(p.solver, 'coarse_is_paged', lambda: True)   # the driver's per-slice Python sweep
    per_slice = p.run(model='nn', nn=3, early_stop=4)
    assert _same(per_slice['u'], native['u']) and per_slice['conv_int'] == native['conv_int']


def test_light_driver_and_checkpoint_resume(gpu, tmp_path):
    full = lorenz_nn_run(gpu)
    light = _lorenz(gpu, gpu.PararealLight)[1].run(model='nn', nn=3, early_stop=3)   # its newest iterate: column 3
    assert light['u'].shape == (33, 3) and _same(light['u'], full['u'][:, :, 3])
    assert light['conv_int'] == full['conv_int'][:3]
    _, p = _lorenz(gpu)
    again = p.run(model='nn', nn=3, early_stop=4, store_int=True, int_dir=str(tmp_path), int_name='kn')
    assert _same(again['u'], full['u'])
    res = _lorenz(gpu)[1].load_int_dump(str(tmp_path / 'kn' / 'kn_1.npz'), early_stop=4)
    assert res['k'] == full['k'] and res['conv_int'] == full['conv_int']
    assert _same(res['u'], full['u']) and _same(res['err'], full['err'])
    assert np.array_equal(res['x'], full['x']) and np.array_equal(res['D'], full['D'])


# ------------------------------------------------------------------------------ the comparison
def _comp(gpu):
    return [gpu.NN(N=32, nn=k) for k in COMP_NN] + [gpu.NNGP_p(n=3, N=32, worker_pool=gpu.MyPool(), nn=10, seed=45)]


def plain_debug_run(gpu, model, early_stop=3):
    return cached('plain_' + model, lambda: _lorenz(gpu)[1].run(model=model, early_stop=early_stop, debug=True))


def _unchanged(r, base):
    assert r['k'] == base['k'] and r['conv_int'] == base['conv_int'] and _same(r['u'], base['u'])
    a, b = r['debug_dict'], base['debug_dict']
    assert np.array_equal(_bits(a['one_step_error']), _bits(b['one_step_error']))
    assert len(a['all_pred_err']) == len(b['all_pred_err'])
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a['all_pred_err'], b['all_pred_err']))


def test_comparison_lists_are_bitwise_the_restatement(gpu):
    r = _lorenz(gpu)[1].run(model='parareal', early_stop=3, debug=True, comp_mdls=_comp(gpu))
    o = _lorenz_ref(model='parareal', early_stop=3, debug=True,
                    comp=[KR.NNRef(k) for k in COMP_NN] + [KR.NNGPRef(3, nn=10, seed=45)])
    _check_run(r, o)
    got, ref = r['err_store_mdls'], o['err_store_mdls']
    assert sorted(got) == sorted(ref) == sorted([f'{k}-NN' for k in COMP_NN] + ['NNGP', 'para'])
    for name in ref:
        assert sorted(got[name]) == sorted(ref[name]) == [0, 1, 2], name
        for k in ref[name]:
            assert len(got[name][k]) == len(ref[name][k]) > 0, (name, k)
            assert np.array_equal(_bits(got[name][k]), _bits(ref[name][k])), (name, k)
    _unchanged(r, plain_debug_run(gpu, 'parareal'))
    assert 'err_store_mdls' not in plain_debug_run(gpu, 'parareal')


def test_comparison_without_debug_fits_and_leaves_the_lists_empty(gpu):
    comp = _comp(gpu)[:2]
    r = _lorenz(gpu)[1].run(model='parareal', early_stop=3, comp_mdls=comp)
    assert _same(r['u'], plain_debug_run(gpu, 'parareal')['u'])
    assert r['err_store_mdls'] == {n: {0: [], 1: [], 2: []} for n in ('1-NN', '2-NN', 'para')}
    assert all(m.k == 2 and m.x.shape == r['x'].shape for m in comp)


def test_comparison_under_the_full_gp_driver(gpu):
    """Figure 2's second panel: the run is unchanged, and the NN lists are the restatement's on this
    run's own x, D and u (the truth F(u_i) - G(u_i) from the oracle's propagators, bitwise the GPU's)."""
    comp = [gpu.NN(N=32, nn=k) for k in COMP_NN]
    r = _lorenz(gpu)[1].run(model='gpjax', early_stop=4, debug=True, comp_mdls=comp)
    _unchanged(r, plain_debug_run(gpu, 'gpjax', early_stop=4))
    so, N, t = O.System('lorenz'), 32, r['t']
    assert r['k'] == 4 and all(len(r['err_store_mdls'][f'{c}-NN'][3]) == N - r['conv_int'][2] - 1 for c in COMP_NN)
    rows = 0
    for k in range(3):   # the result keeps the iterates 0 .. k-1: the last sweep's queries are not in it
        I0 = 0 if k == 0 else r['conv_int'][k - 1]
        rows += N - I0
        I = I0 + 1
        Q = r['u'][I:N, :, k + 1]
        uG = np.array([so.rk(4, t[i], t[i + 1], 6, r['u'][i, :, k + 1]) for i in range(I, N)])
        truth = so.rk_batch(4, t[I:N], t[I + 1:N + 1], 450, Q) - uG
        ref = KR.compare_lists(r['x'][:rows], r['D'][:rows], Q, truth, [KR.NNRef(c) for c in COMP_NN])
        for name in ref:
            assert np.array_equal(_bits(r['err_store_mdls'][name][k]), _bits(ref[name])), (name, k)


def test_user_model_goes_through_the_host_fallback(gpu):
    calls = []

    class Zero(gpu.ModelAbstr):
        name = 'zero'

        def fit(self, x, y, *args, **kwargs):
            assert isinstance(x, np.ndarray) and x.shape == y.shape and 'data_x' in kwargs
            self.rows = x.shape[0]

        def predict(self, new_x, prev_F, prev_G, *args, **kwargs):
            assert new_x.shape == (1, 3) and prev_F.shape == prev_G.shape == (3,) and kwargs['truth'].shape == (3,)
            calls.append(kwargs['i'])
            return np.zeros(3)

    r = _lorenz(gpu)[1].run(model='parareal', early_stop=2, debug=True, comp_mdls=[Zero(N=32), gpu.NN(N=32, nn=2)])
    assert calls == list(range(1, 32)) + list(range(r['conv_int'][0] + 1, 32))
    base = plain_debug_run(gpu, 'parareal')
    assert _same(r['u'], base['u'][:, :, :2])
    # a zero prediction's error is the truth itself: never below the classic update's on this run's first sweep
    assert len(r['err_store_mdls']['zero'][0]) == 31 and np.all(np.isfinite(r['err_store_mdls']['zero'][0]))


def test_figure_2_configuration_matches_the_reference_run(gpu):
    z = golden('knnmean.npz')
    t0, t1, N, Ng, Nf, eps = z['cfg']
    ode = gpu.Rossler(normalization='-11')
    assert np.array_equal(ode.get_init_cond(), z['u0'])
    s = gpu.SolverRK(ode.get_vector_field(), Ng=int(Ng), Nf=int(Nf), F='RK4', G='RK1')
    p = gpu.Parareal(ode, s, [t0, t1], int(N), epsilon=float(eps), verbose=None)
    r = p.run(comp_mdls=[gpu.NN(N=int(N), nn=k) for k in COMP_NN], debug=True)
    assert r['k'] == int(z['b__k']) and r['conv_int'] == list(z['b__conv_int']) and r['converged']
    worst = KR.check_lists_against_fixture(r['err_store_mdls'], z)
    print(f'largest |10**e - 10**e_ref| = {worst:.3e}')
