"""nngp_predict_batch pinned to the single prediction, bitwise.

Query q of a batch is nngp_predict at Q[q] with its own block of theta0: preds, out = preds + bias,
every column of every fit and the ordered neighbour list (nngp_knn) are compared as raw doubles
(NaN positions equal), never within a tolerance -- the batch runs the select, the fits and the mean
on the same device functions, so the operations and their order are the single prediction's.

* every padded fit size at its lower edge and its size (m = 1 ... 64), nq = 1, 2, 17;
* the three places D2 / kd2 come from -- the select itself (d <= 128 on staged rows: sequential
  below d = 8, octets above), a wave per pair (d > 128) and a thread per pair (NNGP_D2_WAVES=0) --
  on both sides of d = 128 / 129 at m = 20;
* against the oracle's own predict, so the chain of trust does not rest on nngp_predict alone;
* ties and edges: duplicated training rows, a query on a training row, rows == m, two restarts,
  a set whose Cholesky fails at the low jitters;
* independence: a permuted batch gives the permuted rows, a query alone gives its batched row;
* the host's chunking: one query more than a chunk holds (d = 288: 2 592 fits per query);
* NNGP_p.predict_batch / predict_batch_device and the driver's model comparison (comp_mdls)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import knn_cases as KC
import nm_cases as NC
import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JIT = np.arange(-20, -11, dtype=float)
SENT = -7.125e77   # what the output buffers hold before a call (no theta, -LML, count or mean is this)


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


def draws(d, nq, R=1, seed=3):
    """theta0 [nq][d*9*R][2]: what a model seeded `seed` draws for nq consecutive predictions."""
    import nngp_amd
    return nngp_amd.NNGP_p(n=d, N=4, nn=10, seed=seed, n_restarts=R).draw_thetas(nq).reshape(nq, d * 9 * R, 2)


def queries(X, nq, seed):
    """nq queries near training rows (so neighbour lists differ from query to query)."""
    rng = np.random.default_rng(seed)
    return X[rng.choice(X.shape[0], size=nq, replace=nq > X.shape[0])] + 0.01 * rng.standard_normal((nq, X.shape[1]))


def batch(gpu, X, Y, Q, m, th0, R=1, bias=None, alias=False, maxfev=400):
    """nngp_predict_batch with every output: dict(preds, out, idx, fits) on the host."""
    import torch
    rows, d = X.shape
    nq, nf = Q.shape[0], d * 9 * R
    assert th0.shape == (nq, nf, 2)
    preds = torch.full((nq, d), SENT, dtype=torch.float64, device='cuda')
    idx = torch.full((nq, m), -7, dtype=torch.int32, device='cuda')
    fits = torch.full((nq, nf, 4), SENT, dtype=torch.float64, device='cuda')
    bt = None if bias is None else _t(bias)
    out = None if bias is None else (bt if alias else torch.full((nq, d), SENT, dtype=torch.float64, device='cuda'))
    Xt, Yt, Qt, tht = _t(X), _t(Y), _t(Q), _t(th0)
    gpu._lib.check(gpu.lib().nngp_predict_batch(
        Xt.data_ptr(), Yt.data_ptr(), rows, d, Qt.data_ptr(), nq, m, 9, _jp(), R, tht.data_ptr(), 0.1, 0.1, maxfev,
        preds.data_ptr(), None if bt is None else bt.data_ptr(), None if out is None else out.data_ptr(),
        idx.data_ptr(), fits.data_ptr(), None))
    torch.cuda.synchronize()
    return dict(preds=preds.cpu().numpy(), out=None if out is None else out.cpu().numpy(), idx=idx.cpu().numpy(),
                fits=fits.cpu().numpy())


def singles(gpu, X, Y, Q, m, th0, R=1, bias=None, maxfev=400):
    """The same outputs from a loop of nngp_predict and nngp_knn, one query per call."""
    import torch
    rows, d = X.shape
    nq, nf = Q.shape[0], d * 9 * R
    L = gpu.lib()
    Xt, Yt, Qt, tht = _t(X), _t(Y), _t(Q), _t(th0)
    preds = torch.full((nq, d), SENT, dtype=torch.float64, device='cuda')
    out = torch.full((nq, d), SENT, dtype=torch.float64, device='cuda')
    idx = torch.full((nq, m), -7, dtype=torch.int32, device='cuda')
    fits = torch.full((nq, nf, 4), SENT, dtype=torch.float64, device='cuda')
    bt = None if bias is None else _t(bias)
    for q in range(nq):
        gpu._lib.check(L.nngp_predict(
            Xt.data_ptr(), Yt.data_ptr(), rows, d, Qt[q].data_ptr(), m, 9, _jp(), R, tht[q].data_ptr(), 0.1, 0.1,
            maxfev, preds[q].data_ptr(), None if bt is None else bt[q].data_ptr(),
            None if bt is None else out[q].data_ptr(), fits[q].data_ptr(), None))
        gpu._lib.check(L.nngp_knn(Xt.data_ptr(), rows, d, Qt[q].data_ptr(), m, idx[q].data_ptr(), None, None))
    torch.cuda.synchronize()
    return dict(preds=preds.cpu().numpy(), out=None if bias is None else out.cpu().numpy(), idx=idx.cpu().numpy(),
                fits=fits.cpu().numpy())


def check_equal(got, want, rows=None):
    """Every output of `got` bitwise `want` (rows: the rows of `want` that `got` holds, in order)."""
    for key in ('preds', 'out', 'fits'):
        if want[key] is None:
            assert got[key] is None
            continue
        w = want[key] if rows is None else want[key][rows]
        assert not np.any(w == SENT) and _same(got[key], w), key
    w = want['idx'] if rows is None else want['idx'][rows]
    assert np.array_equal(got['idx'], w) and w.min() >= 0


# ---------------------------------------------------------------- 1. against the single prediction
EDGE_MS = (1, 8, 9, 15, 16, 17, 20, 24, 32, 33, 48, 64)
NQ_MAX = 17


@functools.lru_cache(maxsize=None)
def edge_case(m):
    """d = 3, rows = 80: (X, Y, Q [17][3], theta0, bias) and the loop of single predictions."""
    X, Y, _ = KC.predict_data((m, 3, 80))
    Q = queries(X, NQ_MAX, 100 + m)
    th0 = draws(3, NQ_MAX)
    bias = np.random.default_rng(m).standard_normal((NQ_MAX, 3))
    return X, Y, Q, th0, bias


_edge_ref = {}


def edge_ref(gpu, m):
    if m not in _edge_ref:
        X, Y, Q, th0, bias = edge_case(m)
        _edge_ref[m] = singles(gpu, X, Y, Q, m, th0, bias=bias)
    return _edge_ref[m]


@pytest.mark.parametrize('nq', [1, 2, NQ_MAX])
@pytest.mark.parametrize('m', EDGE_MS)
def test_batch_is_the_loop_of_single_predictions(gpu, m, nq):
    X, Y, Q, th0, bias = edge_case(m)
    got = batch(gpu, X, Y, Q[:nq], m, th0[:nq], bias=bias[:nq], alias=(nq == 2))
    check_equal(got, edge_ref(gpu, m), rows=slice(0, nq))


def test_optional_outputs_may_be_left_out(gpu):
    """idx_out, fits_out, bias and out all NULL: the same preds (the workspace holds the rest)."""
    import torch
    m = 15
    X, Y, Q, th0, _ = edge_case(m)
    preds = torch.full((NQ_MAX, 3), SENT, dtype=torch.float64, device='cuda')
    Xt, Yt, Qt, tht = _t(X), _t(Y), _t(Q), _t(th0)
    gpu._lib.check(gpu.lib().nngp_predict_batch(
        Xt.data_ptr(), Yt.data_ptr(), 80, 3, Qt.data_ptr(), NQ_MAX, m, 9, _jp(), 1, tht.data_ptr(), 0.1, 0.1, 400,
        preds.data_ptr(), None, None, None, None, None))
    torch.cuda.synchronize()
    assert _same(preds.cpu().numpy(), edge_ref(gpu, m)['preds'])


# ------------------------------------------------------------------------------------ 2. D2 forms
# m = 20 (csrc/nngp_gp.hip d2_by_waves / d2_by_pairs, knn_select_dev): the select computes D2 / kd2
# while d <= 128 and m * (d + 1) <= 6144 (d <= 306 here, so d = 129 is the first d past it) --
# sequentially below d = 8, by octets from d = 8 -- a wave per pair does from d = 129, a thread per
# pair under NNGP_D2_WAVES=0.
D2_CASES = [(7, None), (8, None), (16, None), (128, None), (128, '0'), (129, None), (129, '0'), (200, None),
            (200, '0')]


@pytest.mark.parametrize('d,waves', D2_CASES, ids=[f'd{d}' + ('-pairs' if w else '') for d, w in D2_CASES])
def test_every_d2_form(gpu, d, waves, monkeypatch):
    m, rows, nq = 20, 60, 3
    form = KC.geometry_form(m, d, d2_waves=waves is None)
    assert form == ('sequential' if d < 8 else ('octet' if d <= 128 else ('wave' if waves is None else 'pairs')))
    if waves is not None:
        monkeypatch.setenv('NNGP_D2_WAVES', waves)
    X, Y, _ = KC.predict_data((m, d, rows))
    Q = queries(X, nq, d)
    th0 = draws(d, nq)
    bias = np.random.default_rng(d).standard_normal((nq, d))
    check_equal(batch(gpu, X, Y, Q, m, th0, bias=bias), singles(gpu, X, Y, Q, m, th0, bias=bias))


# ---------------------------------------------------------------------- 3. against the oracle
@pytest.mark.parametrize('d,m', [(3, 15), (16, 20)])
def test_batch_is_the_oracles_prediction(gpu, d, m):
    rows, nq = 60, 3
    X, Y, _ = KC.predict_data((m, d, rows))
    Q = queries(X, nq, 7 * d)
    th0 = draws(d, nq)
    bias = np.random.default_rng(d).standard_normal((nq, d))
    got = batch(gpu, X, Y, Q, m, th0, bias=bias)
    for q in range(nq):
        preds, fits = O.predict(X, Y, Q[q], m, th0[q], return_fits=True)
        assert _same(got['preds'][q], preds) and _same(got['fits'][q], fits), q
        assert _same(got['out'][q], preds + bias[q]), q
        assert np.array_equal(got['idx'][q], O.knn(X, Q[q], m)[0]), q


# ------------------------------------------------------------------------------ 4. ties and edges
def test_duplicated_training_rows_and_a_query_on_one(gpu):
    """30 copies of one training row (the select's index tie-break; singular kernel matrices), one
    query on that row, one on another training row, the rest nearby."""
    m = 15
    X, Y, q = KC.predict_data((m, 3, 80, 30))
    src = X[80 // 3]
    assert np.count_nonzero((X == src).all(axis=1)) >= 30
    Q = np.vstack([src, X[5], q, queries(X, 2, 9)])
    th0 = draws(3, len(Q))
    want = singles(gpu, X, Y, Q, m, th0)
    dup = np.flatnonzero((X == src).all(axis=1))
    assert np.array_equal(want['idx'][0], dup[:m])          # an all-tie list: by index
    check_equal(batch(gpu, X, Y, Q, m, th0), want)


def test_every_row_is_a_neighbour_and_two_restarts(gpu):
    m = rows = 20
    X, Y, _ = KC.predict_data((m, 3, rows))
    Q = queries(X, 4, 11)
    th0 = draws(3, 4, R=2)
    assert th0.shape == (4, 54, 2)
    want = singles(gpu, X, Y, Q, m, th0, R=2)
    assert all(sorted(r) == list(range(rows)) for r in want['idx'])
    check_equal(batch(gpu, X, Y, Q, m, th0, R=2), want)


@pytest.mark.parametrize('m', [20, 33])
def test_failed_factorisations_give_the_single_calls_fits_and_argmin(gpu, m):
    """nm_cases' 'dup' set: two neighbours coincide, so the Cholesky fails at low jitters -- by the
    oracle some fits of the first query start on a failed factorisation (-LML = +inf), simplices mix
    +inf and finite vertices, and the batch's fits and arg-min are still the single call's."""
    X, Y, q, _ = NC.predict_case(m, 'dup')
    Q = np.vstack([q, X[m // 2], q + 0.003])
    th0 = draws(3, len(Q), seed=2000 + m)
    nb = O.knn(X, q, m)[0]
    D2 = O.d2_matrix(X[nb])
    start = [O.nlml(D2, Y[nb][:, f // 9], th0[0][f], float(JIT[f % 9])) for f in range(27)]
    assert not np.isfinite(start).all()                     # the case does fail somewhere
    want = singles(gpu, X, Y, Q, m, th0)
    check_equal(batch(gpu, X, Y, Q, m, th0), want)


# ------------------------------------------------------------------------------ 5. independence
def test_permuted_queries_give_permuted_rows_and_a_query_alone_its_row(gpu):
    m = 15
    X, Y, Q, th0, bias = edge_case(m)
    want = edge_ref(gpu, m)
    perm = np.random.default_rng(5).permutation(NQ_MAX)
    assert not np.array_equal(perm, np.arange(NQ_MAX))
    check_equal(batch(gpu, X, Y, Q[perm], m, th0[perm], bias=bias[perm]), want, rows=perm)
    for q in (0, 9, NQ_MAX - 1):
        check_equal(batch(gpu, X, Y, Q[q:q + 1], m, th0[q:q + 1], bias=bias[q:q + 1]), want, rows=slice(q, q + 1))


# ---------------------------------------------------------------------------------- 6. chunk edge
def test_one_query_past_a_chunk(gpu):
    """d = 288 (FHN-PDE nx = 12), m = 10, rows = 30: 2 592 fits per query, 101 queries per chunk by
    the header's constant; 102 queries make a second chunk of one."""
    src = open(os.path.join(ROOT, 'include', 'nngp.h')).read()
    bound = int(re.search(r'^#define\s+NNGP_PREDICT_BATCH_MAX_FITS\s+(\d+)', src, re.M).group(1))
    d, m, rows = 288, 10, 30
    chunk = min(65535, max(1, bound // (d * 9)))
    nq = chunk + 1
    assert (chunk, nq) == (101, 102)
    X, Y, _ = KC.predict_data((m, d, rows))
    Q = queries(X, nq, 288)
    th0 = draws(d, nq)
    bias = np.random.default_rng(288).standard_normal((nq, d))
    got = batch(gpu, X, Y, Q, m, th0, bias=bias)
    assert not np.any(got['preds'] == SENT) and not np.any(got['fits'] == SENT) and got['idx'].min() >= 0
    look = np.array([0, chunk - 2, chunk - 1, chunk])       # first | the boundary's two sides | last
    check_equal({k: v[look] for k, v in got.items()}, singles(gpu, X, Y, Q[look], m, th0[look], bias=bias[look]))


# -------------------------------------------------------------------------------------- 7. Python
def test_model_predict_batch_is_the_loop_of_predict(gpu):
    d, rows, nq = 3, 80, 6
    X, Y, _ = KC.predict_data((12, d, rows))
    Q = queries(X, nq, 21)
    a = gpu.NNGP_p(n=d, N=4, nn=12, seed=9)
    b = gpu.NNGP_p(n=d, N=4, nn=12, seed=9)
    a.fit(X, Y, 0)
    b.fit(X, Y, 0)
    got = a.predict_batch(Q)
    want = np.array([b.predict(Q[j]) for j in range(nq)])
    assert got.shape == (nq, d) and _same(got, want)
    assert a.train_count == b.train_count == nq * a.n_fits == nq * 27
    # the streams stay together: the next draw of either model is the same
    assert np.array_equal(a.draw_thetas(1), b.draw_thetas(1))
    # more neighbours than rows keep every row, as predict does
    c, e = gpu.NNGP_p(n=d, N=4, nn=30, seed=1), gpu.NNGP_p(n=d, N=4, nn=30, seed=1)
    c.fit(X[:20], Y[:20], 0)
    e.fit(X[:20], Y[:20], 0)
    assert _same(c.predict_batch(Q[:2]), np.array([e.predict(Q[j]) for j in range(2)]))
    assert a.predict_batch(np.empty((0, d))).shape == (0, d) and a.train_count == nq * 27


def test_comparison_nngps_predict_each_iteration_in_one_call(gpu, monkeypatch):
    """Lorenz N = 8 under the classic driver with two comparison nnGPs: their err_store_mdls lists are
    what per-slice predict_device calls of equally seeded twins give on the run's own iterates and
    training history, and each model made ONE nngp_predict_batch call per iteration."""
    import torch
    N, Ng, Nf, K = 8, 6, 60, 3
    ode = gpu.Lorenz(normalization='-11')
    s = gpu.SolverRK(ode.get_vector_field(), Ng=Ng, Nf=Nf, F='RK4', G='RK4')
    p = gpu.Parareal(ode, s, [0, 4.5], N, epsilon=5e-7, verbose=None)
    mk = lambda: [gpu.NNGP_p(n=3, N=N, nn=10, seed=45), gpu.NNGP_p(n=3, N=N, nn=12, seed=46)]
    comp, twins = mk(), mk()
    for mdl, name in zip(comp, ('NNGP10', 'NNGP12')):
        mdl.name = name                                     # (err_store_mdls is keyed by name)
    L = gpu.lib()
    calls = []
    real = L.nngp_predict_batch

    def counted(*args):
        calls.append(int(args[5]))                          # n_q
        return real(*args)

    monkeypatch.setattr(L, 'nngp_predict_batch', counted)
    r = p.run(model='parareal', early_stop=K + 1, debug=True, comp_mdls=comp)
    monkeypatch.undo()
    lists = r['err_store_mdls']
    assert sorted(lists) == ['NNGP10', 'NNGP12', 'para']
    compared = [k for k in sorted(lists['NNGP10']) if len(lists['NNGP10'][k])]
    assert compared == list(range(len(compared))) and len(calls) == 2 * len(compared)
    t = r['t']
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')
    rows, n_iter = 0, 0
    for k in range(min(K, r['k'] - 1)):   # (the result keeps the iterates up to the last sweep's start)
        I0 = 0 if k == 0 else r['conv_int'][k - 1]
        rows += N - I0
        I = I0 + 1
        if I >= N:
            break
        n_iter += 1
        nq = N - I
        Qh = np.ascontiguousarray(r['u'][I:N, :, k + 1])
        Q, t0, t1 = dev(Qh), dev(t[I:N]), dev(t[I + 1:N + 1])
        truth = s.run_F_batch(t0, t1, Q).cpu().numpy() - s.run_G_batch(t0, t1, Q).cpu().numpy()
        Xd, Yd = dev(r['x'][:rows]), dev(r['D'][:rows])
        for mdl, twin in zip(comp, twins):
            twin.fit(Xd, Yd, k)
            th0 = dev(twin.draw_thetas(nq))
            nf = twin.n_fits
            P = torch.empty((nq, 3), dtype=torch.float64, device='cuda')
            for j in range(nq):
                twin.predict_device(Xd, Yd, rows, Q[j], th0[j * nf:(j + 1) * nf], preds=P[j])
            Ph = P.cpu().numpy()
            with np.errstate(divide='ignore'):
                want = [float(np.max(np.log10(np.abs(truth[j] - Ph[j])))) for j in range(nq)]
            got = lists[mdl.name][k]
            assert len(got) == nq and _same(got, want), (mdl.name, k)
            assert calls[2 * k + comp.index(mdl)] == nq
    assert n_iter >= 2
