"""CPU: the k-NN Parareal contract's restatement (tests/knnmean_ref.py) against the
reference's own NN model and Figure 2 comparison loop (tests/golden/knnmean.npz, written by
tests/golden/gen_knnmean.py), the Python surface of models.NN / comp_mdls without a GPU, and the
argument checks of the two C entry points."""
import ctypes

import numpy as np
import pytest

import knnmean_ref as KR
import oracle as O
from conftest import golden

PRED_D, PRED_NN, PRED_ROWS = (2, 3, 33), (1, 2, 8, 9, 30, 64), (5, 40, 300)
COMP_NN = KR.COMP_NN


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------- the contract
@pytest.mark.parametrize('d', PRED_D)
@pytest.mark.parametrize('rows', PRED_ROWS)
def test_restatement_is_bitwise_the_reference_predict(d, rows):
    z = golden('knnmean.npz')
    tag = f'a__d{d}_r{rows}'
    X, Y, q = z[tag + '__X'], z[tag + '__Y'], z[tag + '__q']
    counts = [min(nn, rows) for nn in PRED_NN]   # rows = 5 < nn: the reference keeps every row
    got = KR.knn_mean(X, Y, q, counts)
    for j, nn in enumerate(PRED_NN):
        ref = z[tag + f'__pred_nn{nn}']
        assert np.array_equal(_bits(got[j]), _bits(ref)), (nn, np.max(np.abs(got[j] - ref)))
        alone = KR.knn_mean(X, Y, q, [counts[j]])[0]   # a count's bits do not depend on the others
        assert np.array_equal(_bits(alone), _bits(ref))


def test_d1_mean_is_the_sequential_sum():
    """The one documented deviation: for d = 1 and m >= 8 NumPy's mean sums pairwise; the contract
    stays sequential.  Y = [1e16, 1, -1e16, 1, ...] in neighbour order: left to right the ones are
    absorbed by 1e16 (a sum of 1), pairwise they are not all."""
    m = 9
    X = np.arange(m, dtype=np.float64).reshape(m, 1)          # distances 0, 1, 4, ..: the order is the row order
    Y = np.array([1e16, 1.0, -1e16, 1.0, 1e16, 1.0, -1e16, 1.0, 1.0]).reshape(m, 1)
    s = Y[0, 0]
    for r in range(1, m):
        s = s + Y[r, 0]
    got = KR.knn_mean(X, Y, np.zeros(1), [m])[0]
    assert got[0] == s / 9.0
    assert Y.mean(axis=0)[0] != got[0]   # NumPy's collapsed 1-D reduction is the pairwise sum


def test_counts_unsorted_with_repeats_and_nonfinite_rows():
    rng = np.random.default_rng(3)
    X, Y = rng.standard_normal((50, 4)), rng.standard_normal((50, 4))
    q = X[7] + 1e-3
    idx = KR.knn_mean_idx(X, q, 30)
    Y[idx[2], 1] = np.nan
    Y[idx[5], 2] = np.inf
    counts = [10, 1, 30, 4, 1]
    got = KR.knn_mean(X, Y, q, counts)
    assert np.array_equal(_bits(got[1]), _bits(got[4])) and np.array_equal(_bits(got[1]), _bits(Y[idx[0]]))
    assert np.isnan(got[0, 1]) and np.isinf(got[0, 2]) and np.isfinite(got[3, 2]) and np.isfinite(got[1]).all()
    four = (((Y[idx[0]] + Y[idx[1]]) + Y[idx[2]]) + Y[idx[3]]) / 4.0   # the NaN row is among the first four
    assert np.isnan(four[1]) and np.array_equal(got[3], four, equal_nan=True)


# ---------------------------------------------------------------------- the comparison loop
_loops = {}


def restated(which):
    """The restated loop on the fixture's configuration, computed once and left unchanged."""
    if which not in _loops:
        z = golden('knnmean.npz')
        t0, t1, N, Ng, Nf, eps = z['cfg']
        kw = dict(epsilon=float(eps), u0=z['u0'])
        so = O.System('rossler')
        if which == 'b':
            kw.update(model='parareal', comp=[KR.NNRef(k) for k in COMP_NN], debug=True)
        else:
            kw.update(model='nn', nn=3)
        _loops[which] = KR.parareal_compare(so, [t0, t1], int(N), int(Ng), int(Nf), 'RK1', 'RK4', **kw)
        _loops[which]['u'].setflags(write=False)
    return _loops[which]


def test_restated_comparison_loop_matches_the_reference_run():
    z = golden('knnmean.npz')
    o = restated('b')
    assert o['k'] == int(z['b__k']) and o['conv_int'] == list(z['b__conv_int'])
    assert np.nanmax(np.abs(o['u'] - z['b__u'])) < 1e-9   # the Parareal-run bound of test_oracle_golden.py
    worst = KR.check_lists_against_fixture(o['err_store_mdls'], z)
    print(f'largest |10**e - 10**e_ref| = {worst:.3e} (fixture max_abs_dev = {float(z["max_abs_dev"]):.3e})')
    # the nearest row of a slice's starting value is its own previous iterate: 1-NN = classic Parareal early on
    assert o['err_store_mdls']['1-NN'][0] == o['err_store_mdls']['para'][0]


def test_restated_knn_driver_matches_the_reference_run():
    z = golden('knnmean.npz')
    o = restated('c')
    assert o['k'] == int(z['c__k']) and o['conv_int'] == list(z['c__conv_int'])
    assert np.max(np.abs(o['u'][:, :, -1] - z['c__u'][:, :, -1])) < 1e-9   # test_oracle_golden.py's bound


# ----------------------------------------------------------------------- the Python surface
def test_names_defaults_and_refusals():
    import nngp_amd
    assert 'NN' in nngp_amd.__all__ and issubclass(nngp_amd.NN, nngp_amd.ModelAbstr)
    m = nngp_amd.NN(N=8)
    assert m.nn == 10 and m.name == '10-NN' and m.pred_times.shape == (8,)
    assert nngp_amd.NN(N=8, nn=3).name == '3-NN' and nngp_amd.NN(N=8, nn=64).nn == 64
    with pytest.raises(ValueError, match='64'):
        nngp_amd.NN(N=8, nn=65)
    with pytest.raises(ValueError, match='nn'):
        nngp_amd.NN(N=8, nn=0)
    with pytest.raises(ValueError, match='adaptive'):
        nngp_amd.NN(N=8, nn='adaptive')
    with pytest.raises(ValueError, match='integer'):
        nngp_amd.NN(N=8, nn=2.5)
    with pytest.raises(AttributeError, match='fit'):
        m.x
    x, y = np.zeros((4, 3)), np.ones((4, 3))
    m.fit(x, y, 2, data_x=None, data_y=None)
    assert m.x is x and m.y is y and m.k == 2
    st = m.state_dict()
    assert st['name'] == '10-NN' and st['settings'] == {'nn': 10}
    m2 = nngp_amd.NN(N=8, **st['settings'])
    m2.load_state(st)
    assert m2.k == 2 and m2.name == m.name
    c = m.store()
    assert c is not m and c.nn == 10 and np.array_equal(c.x, x)


def _small_parareal():
    import nngp_amd
    ode = nngp_amd.Lorenz(normalization='-11')
    s = nngp_amd.SolverRK(ode.get_vector_field(), Ng=6, Nf=45, F='RK4', G='RK4')
    return nngp_amd.Parareal(ode, s, [0, 18], 4, verbose=None)


def test_driver_refuses_bad_neighbour_counts_before_any_gpu_work():
    p = _small_parareal()
    with pytest.raises(ValueError, match='64'):
        p.run(model='nn', nn=65)
    with pytest.raises(ValueError, match='adaptive'):
        p.run(model='nn', nn='adaptive')
    assert p.runs == {}


def test_product_path_fails_loudly_without_gpu():
    """No CPU fallback for the new model or the comparison (the result key itself is checked where a
    run exists: tests/test_gpu_knnmean.py)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    import nngp_amd
    p = _small_parareal()
    with pytest.raises(nngp_amd.NNGPError):
        p.run(model='nn', nn=4)
    with pytest.raises(nngp_amd.NNGPError):
        p.run(comp_mdls=[nngp_amd.NN(N=4, nn=2)], debug=True)
    with pytest.raises(nngp_amd.NNGPError):
        nngp_amd.NN(N=4, nn=2).predict(np.zeros((1, 3)), None, None, i=0)
    assert p.runs == {}


def test_several_ranks_are_refused(monkeypatch):
    import nngp_amd
    ode = nngp_amd.Lorenz(normalization='-11')
    s = nngp_amd.SolverRK(ode.get_vector_field(), Ng=6, Nf=45, F='RK4', G='RK4')
    p = nngp_amd.Parareal(ode, s, [0, 18], 4, verbose=None)
    monkeypatch.setattr(p, '_world', lambda: 2)
    with pytest.raises(NotImplementedError, match="model='nn' runs on one rank"):
        p.run(model='nn', nn=4)
    monkeypatch.setattr(nngp_amd._lib, 'require_gpu', lambda: __import__('torch'))
    with pytest.raises(NotImplementedError, match='comp_mdls runs on one rank'):
        p.run(comp_mdls=[nngp_amd.NN(N=4, nn=2)], debug=True)
    with pytest.raises(TypeError, match='ModelAbstr'):
        p.run(comp_mdls=[object()], debug=True)


# ------------------------------------------------------------------------------------ C-ABI
def test_knn_mean_argument_errors_without_a_device():
    import nngp_amd
    L = nngp_amd.lib()
    P = 64   # any non-null address: every check comes before the first HIP call
    cnt = lambda *v: (ctypes.c_int32 * len(v))(*v)

    def call(X=P, Y=P, rows=100, d=3, Q=P, n_q=5, m=cnt(3), n_m=1, out=P, idx=None, bias=None, ob=None):
        rc = L.nngp_knn_mean(X, Y, rows, d, Q, n_q, m, n_m, out, idx, bias, ob, None)
        return rc, L.nngp_last_error()

    for kw, word in [(dict(X=None), b'X is NULL'), (dict(Y=None), b'Y is NULL'), (dict(Q=None), b'Q is NULL'),
                     (dict(m=None), b'm_host is NULL'), (dict(out=None), b'out is NULL'),
                     (dict(d=0), b'd must be >= 1'), (dict(rows=0), b'rows must be >= 1'),
                     (dict(m=cnt(0)), b'm must be in 1..min(64, rows)'),
                     (dict(m=cnt(65)), b'm must be in 1..min(64, rows)'),
                     (dict(m=cnt(3, 41), n_m=2, rows=40), b'm must be in 1..min(64, rows)'),
                     (dict(n_m=0), b'n_m must be in 1..16'), (dict(m=cnt(*[1] * 17), n_m=17), b'n_m must be in 1..16'),
                     (dict(n_q=-1), b'n_q must be in 0..65535'), (dict(n_q=65536), b'n_q must be in 0..65535'),
                     (dict(bias=P), b'bias and out_biased go together'),
                     (dict(bias=P, ob=P), b'bias needs n_q == n_m == 1'),
                     (dict(bias=P, ob=P, n_q=1, m=cnt(1, 2), n_m=2), b'bias needs n_q == n_m == 1')]:
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    assert call(n_q=0)[0] == 0
    assert call(n_q=0, m=cnt(10, 1, 30, 4, 1), n_m=5)[0] == 0


def test_knn_mean_sweep_argument_errors_without_a_device():
    import nngp_amd
    L = nngp_amd.lib()
    P = 64
    cs = nngp_amd._lib.CSystem(0, 3, 0, 0, (ctypes.c_double * 4)(), None)

    def call(sys=ctypes.byref(cs), t=P, I=1, N=8, U1=P, UG1=P, X=P, Y=P, rows=100, m=3):
        rc = L.nngp_knn_mean_sweep(sys, 4, 0, 6, t, I, N, U1, UG1, X, Y, rows, m, None, None, None)
        return rc, L.nngp_last_error()

    for kw, word in [(dict(sys=None), b'sys is NULL'), (dict(t=None), b't is NULL'), (dict(U1=None), b'U1 is NULL'),
                     (dict(UG1=None), b'UG1 is NULL'), (dict(X=None), b'X is NULL'), (dict(Y=None), b'Y is NULL'),
                     (dict(rows=0), b'rows must be >= 1'), (dict(m=0), b'm must be in 1..min(64, rows)'),
                     (dict(m=65), b'm must be in 1..min(64, rows)'),
                     (dict(m=11, rows=10), b'm must be in 1..min(64, rows)'), (dict(I=-1), b'I must be >= 0')]:
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    cs0 = nngp_amd._lib.CSystem(0, 0, 0, 0, (ctypes.c_double * 4)(), None)
    rc, msg = call(sys=ctypes.byref(cs0))
    assert rc == -1 and b'd must be >= 1' in msg
    assert call(I=8, N=8)[0] == 0 and call(I=9, N=8)[0] == 0   # N <= I: nothing to do


def test_legacy_driver_keeps_refusing():
    import nngp_amd
    ode = nngp_amd.Lorenz(normalization='-11')
    s = nngp_amd.legacy.Parareal(f=ode.get_vector_field(), tspan=[0, 18], u0=ode.get_init_cond(), N=4, Ng=24, Nf=240,
                                 epsilon=5e-7, F='RK4', G='RK4', ode_name='lorenz', verbose=None)
    with pytest.raises(Exception, match='Not implemented'):
        s.run(model='nn', nn=3)
    with pytest.raises(NotImplementedError, match='comp_mdls'):
        s.run(comp_mdls=[nngp_amd.NN(N=4, nn=2)], debug=True)
