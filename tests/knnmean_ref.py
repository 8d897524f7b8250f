"""The k-NN Parareal correction's arithmetic contract restated in NumPy, and the
Parareal loop with the Figure 2 model comparison on it.  Not a test module: shared by
tests/test_knnmean_host.py (CPU) and tests/test_gpu_knnmean.py (GPU).

Contract, for a query q[d], training rows X, Y [rows][d] and a count 1 <= m <= min(64, rows):
  neighbours  i_0 .. i_{m-1} = nngp_knn's list = tests/knn_cases.py::ref_knn (column-ordered sum of
              squares, ascending by (distance, row), NaN last);
  mean        per coordinate c: s = Y[i_0][c]; s = s + Y[i_r][c] for r = 1 .. m-1 in that order;
              out[c] = s / float(m).  No other association, no fma; NaN / inf propagate as IEEE does.
  counts      several counts share one select at max(m_j): the mean for m_j is the running sum after
              m_j rows over m_j -- bitwise the single-count result, because the (distance, row) order
              is total.
This is the reference's ym.mean(axis=0) (Figure_2.py:472-475) bit for bit for d >= 2 (NumPy reduces the
outer axis row by row); for d = 1 and m >= 8 NumPy sums pairwise and the contract stays sequential."""
import numpy as np

from knn_cases import ref_knn

MAX_M = 64
COMP_NN = (1, 2, 4, 10)   # the comparison models of tests/golden/knnmean.npz (gen_knnmean.py)


def knn_mean(X, Y, q, counts, return_idx=False):
    """[len(counts)][d]: the contract's means of the counts[j] nearest rows of (X, Y) at q (and the
    ordered neighbour list at max(counts))."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    counts = [int(c) for c in counts]
    assert all(1 <= c <= min(MAX_M, X.shape[0]) for c in counts), counts
    idx = ref_knn(X, q, max(counts))[0]
    out = np.empty((len(counts), Y.shape[1]))
    with np.errstate(all='ignore'):
        s = None
        for r, i in enumerate(idx):
            s = Y[i].copy() if r == 0 else s + Y[i]
            for j, c in enumerate(counts):
                if c == r + 1:
                    out[j] = s / float(c)
    return (out, idx) if return_idx else out


def knn_mean_idx(X, q, m):
    return ref_knn(X, q, m)[0]


class NNRef:
    """models.NN on the contract (name f'{nn}-NN', the count clamped to the rows at hand)."""

    def __init__(self, nn=10):
        self.nn, self.name = int(nn), f'{int(nn)}-NN'

    def fit(self, x, y, k):
        self.x, self.y = x, y

    def predict(self, q):
        return knn_mean(self.x, self.y, q, [min(self.nn, self.x.shape[0])])[0]


class NNGPRef:
    """An NNGP_p-like comparison entry: the oracle's prediction with its own default_rng(seed), one
    draw of thetas per prediction in slice order (models.py:114, :192)."""

    def __init__(self, n, nn=10, seed=45, name='NNGP', n_restarts=1, fatol=0.1, xatol=0.1):
        self.n, self.nn, self.name = n, nn, name
        self.n_restarts, self.fatol, self.xatol = n_restarts, fatol, xatol
        self.rng = np.random.default_rng(seed)

    def fit(self, x, y, k):
        self.x, self.y, self.k = x, y, k

    def predict(self, q):
        import oracle as O
        m = max(10, self.k + 2) if self.nn == 'adaptive' else self.nn
        m = min(m, self.x.shape[0])
        nf = self.n * len(O.JITTERS) * self.n_restarts
        th0 = self.rng.integers(-8, 0, (nf, 2)).astype(float)
        return O.predict(self.x, self.y, q, m, th0, self.n_restarts, self.fatol, self.xatol)


def log_err(truth, pred):
    """Figure_2.py:202: max_c log10 |truth_c - pred_c| (an exact hit gives -inf)."""
    with np.errstate(divide='ignore'):
        return float(np.max(np.log10(np.abs(truth - pred))))


def compare_lists(x, D, queries, truths, comp):
    """The comparison lists of one iteration for already-fitted entries on given data: used where a
    run's own x, D and iterate are the inputs (a driver model this file does not restate)."""
    out = {}
    for c in comp:
        c.fit(x, D, 0)
        out[c.name] = [log_err(truths[j], c.predict(queries[j])) for j in range(len(queries))]
    return out


def parareal_compare(system, tspan, N, Ng, Nf, G, F, epsilon=5e-7, u0=None, early_stop=None, model='parareal',
                     nn=10, seed=45, comp=None, debug=False):
    """The Parareal loop of oracle.parareal (parareal.py:212-471) restated with the oracle's rk /
    rk_batch / predict, the k-NN model as a driver option (model = 'parareal' | 'nn' | 'nngp') and
    the debug comparison of Figure_2.py:162-203: comp is a list of NNRef / NNGPRef entries, each
    fitted on (x, D) every iteration and, with debug, asked at every slice's starting value
    u[i, :, k+1]; the truth is F(u_i) - uG_new.  Returns oracle.parareal's dict plus
    'err_store_mdls' (when comp is given) and 'all_pred_err' (with debug)."""
    import oracle as O
    n = system.d
    order = {'RK1': 1, 'RK2': 2, 'RK4': 4, 'RK8': 8}
    oG, oF = order[G], order[F]
    t = np.linspace(tspan[0], tspan[1], num=N + 1)
    u0 = np.asarray(u0, dtype=float)
    drv = NNRef(nn) if model == 'nn' else (NNGPRef(n, nn=nn, seed=seed) if model == 'nngp' else None)
    u = np.full((N + 1, n, N + 1), np.nan)
    uG = np.full((N + 1, n, N + 1), np.nan)
    uF = np.full((N + 1, n, N + 1), np.nan)
    err = np.full((N + 1, N), np.nan)
    x = np.zeros((0, n))
    D = np.zeros((0, n))
    conv_int = []
    store = None
    if comp is not None:
        store = {c.name: {} for c in comp}
        store['para'] = {}
    all_pred_err = []
    u[0] = u0[:, None]
    uG[0] = u[0]
    uF[0] = u[0]
    temp = u0
    for i in range(N):
        temp = system.rk(oG, t[i], t[i + 1], Ng, temp, O.STEP_FIXED)
        uG[i + 1, :, 0] = temp
    u[:, :, 0] = uG[:, :, 0]
    I = 0
    for k in range(N):
        uF[I + 1:N + 1, :, k] = system.rk_batch(oF, t[I:N], t[I + 1:N + 1], Nf, u[I:N, :, k], O.STEP_FIXED)
        uG[I + 1, :, k + 1:] = uG[I + 1, :, k].reshape(-1, 1)
        uF[I + 1, :, k + 1:] = uF[I + 1, :, k].reshape(-1, 1)
        u[I + 1, :, k + 1:] = uF[I + 1, :, k].reshape(-1, 1)
        I = I + 1
        x = np.vstack([x, u[I - 1:N, :, k]])
        D = np.vstack([D, uF[I:N + 1, :, k] - uG[I:N + 1, :, k]])
        if I == N:
            err[:, k] = np.linalg.norm(u[:, :, k + 1] - u[:, :, k], np.inf, 1)
            err[-1, k] = np.nextafter(epsilon, 0)
            break
        if drv is not None:
            drv.fit(x, D, k)
        if comp is not None:
            for c in comp:
                store[c.name][k] = []
                store['para'][k] = []
                c.fit(x, D, k)
        preds_t = np.empty((N - I, n))
        for i in range(I, N):
            uG[i + 1, :, k + 1] = system.rk(oG, t[i], t[i + 1], Ng, u[i, :, k + 1], O.STEP_FIXED)
            preds = uF[i + 1, :, k] - uG[i + 1, :, k] if drv is None else drv.predict(u[i, :, k + 1])
            preds_t[i - I] = preds
            u[i + 1, :, k + 1] = preds + uG[i + 1, :, k + 1]
        if debug:
            # every slice's truth in one batch: the comparison reads nothing the sweep has not written
            truth = system.rk_batch(oF, t[I:N], t[I + 1:N + 1], Nf, u[I:N, :, k + 1], O.STEP_FIXED) - \
                uG[I + 1:N + 1, :, k + 1]
            all_pred_err.append(np.abs(truth - preds_t))
            if comp is not None:
                for c in comp:   # model by model, slices in order: an entry's rng stream is its own
                    store[c.name][k] = [log_err(truth[i - I], c.predict(u[i, :, k + 1])) for i in range(I, N)]
                store['para'][k] = [log_err(truth[i - I], preds_t[i - I]) for i in range(I, N)]
        if np.any(np.isnan(uG[:, :, k + 1])):
            raise Exception('NaN values in initial coarse solve - increase Ng!')
        err[:, k] = np.linalg.norm(u[:, :, k + 1] - u[:, :, k], np.inf, 1)
        err[I, k] = 0
        II = I
        for p in range(II + 1, N + 1):
            if err[p, k] < epsilon:
                u[p, :, k + 2:] = u[p, :, k + 1].reshape(-1, 1)
                uG[p, :, k + 2:] = uG[p, :, k + 1].reshape(-1, 1)
                uF[p, :, k + 1:] = uF[p, :, k].reshape(-1, 1)
                I = I + 1
            else:
                break
        conv_int.append(I)
        if I == N:
            break
        if early_stop is not None and k == early_stop - 1:
            break
    out = {'t': t, 'u': u[:, :, :k + 1], 'err': err[:, :k + 1], 'k': k + 1, 'x': x, 'D': D,
           'converged': I == N, 'conv_int': conv_int}
    if store is not None:
        out['err_store_mdls'] = store
    if debug:
        out['all_pred_err'] = all_pred_err
    return out


def check_lists_against_fixture(store, z):
    """Every list of the reference's comparison run (tests/golden/knnmean.npz, group b): the same
    iterations and lengths, and |10**e - 10**e_ref| <= 10 * max_abs_dev for every entry (-inf on both
    sides or on neither).  Returns the largest deviation."""
    bound = 10.0 * float(z['max_abs_dev'])
    worst = 0.0
    for name in [f'{k}-NN' for k in COMP_NN] + ['para']:
        its = [int(k) for k in z[f'b__iters__{name}']]
        assert sorted(store[name]) == its, name
        for k in its:
            ref = z[f'b__err__{name}__{k}']
            got = np.array(store[name][k], dtype=float)
            assert got.shape == ref.shape, (name, k)
            assert np.array_equal(np.isneginf(got), np.isneginf(ref)), (name, k)
            dev = np.abs(10.0 ** got - 10.0 ** ref)
            worst = max(worst, float(dev.max()) if dev.size else 0.0)
            assert np.all(dev <= bound), (name, k, float(dev.max()), bound)
    return worst
