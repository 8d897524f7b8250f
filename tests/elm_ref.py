"""NumPy restatement of the ELM arithmetic contract: the random-weights feature
map in the summation order of csrc/nngp_elm.hip (elm_hidden_kernel), the Gram-Schmidt solve of
elm_solve_kernel, and a Parareal loop with this model on the oracle's propagators and kNN.  It is
the bitwise yardstick of tests/test_gpu_elm.py and tests/test_gpu_elm_forms.py, itself checked on the
CPU against the reference's ELM_base (tests/test_elm_host.py, tests/golden/elm.npz, elm_wide.npz).  NumPy's elementwise fp64 add / sub / mul
/ div / sqrt are IEEE, one rounding per operation, so this is bit-reproducible.  Not a test module
(no test_ prefix)."""
import os
import sys
from itertools import combinations_with_replacement

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle'))

TAU = 2.0 ** -8      # csrc/nngp_elm.h NNGP_ELM_TAU: a row is kept iff |r|^2 > TAU * |z|^2
TAU_EXACT = 2.0 ** -52   # the threshold's starting value: only rows the reference's Gram arithmetic has lost drop
CHUNK = 1024         # csrc/nngp_elm.h ELM_CHUNK: features per partial sum
LANES = 64


def n_poly(d, degree):
    """Number of PolynomialFeatures(degree) columns of a d-vector, degree 1 or 2."""
    return 1 + d + (d * (d + 1) // 2 if degree == 2 else 0)


def feature_pairs(d):
    """The (i, j) of the degree-2 columns, in sklearn's combinations_with_replacement order."""
    return list(combinations_with_replacement(range(d), 2))


def features(x, degree=2):
    """phi(x): 1, x_0 .. x_{d-1}, then x_i * x_j for i <= j (row i: (i,i), (i,i+1), .. (i,d-1))."""
    x = np.asarray(x, dtype=np.float64)
    parts = [np.ones(1), x]
    if degree == 2:
        parts += [x[i] * x[i:] for i in range(len(x))]
    return np.concatenate(parts)


def draw_weights(d, seed=47, res_size=20, degree=2, R=1):
    """ELM_base.__init__ / predict (models.py:481-504, 524): bias, then C, from default_rng(seed);
    C scaled by R.  Returns bias [res_size], C [res_size][n_poly]."""
    rng = np.random.default_rng(seed)
    bias = rng.uniform(-1, 1, (res_size, 1))
    C = rng.uniform(-1, 1, (res_size, n_poly(d, degree)))
    return bias[:, 0].copy(), R * C


def hidden(X, bias, C, degree=2):
    """H[row][r] = relu(bias[r] + sum_f C[r][f] * phi_f(x_row)) in the kernel's order: the features
    in chunks of CHUNK; inside a chunk lane l adds C*phi of features base+l, base+l+64, .. in
    ascending order onto 0.0; the 64 lane sums combine by the xor butterfly 1, 2, 4, 8, 16, 32
    (v = v + v[lane ^ off]); the chunk sums add in ascending chunk order, left to right; then
    bias + total and relu as (v > 0 ? v : 0)."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    res, F = C.shape
    nch = (F + CHUNK - 1) // CHUNK
    lane = np.arange(LANES)
    H = np.empty((X.shape[0], res))
    P = np.zeros((res, nch * CHUNK))
    for n, x in enumerate(X):
        P[:, :F] = C * features(x, degree)[None, :]   # the tail stays +0.0: v + 0.0 == v, v never -0.0
        Pc = P.reshape(res, nch, CHUNK // LANES, LANES)
        acc = np.zeros((res, nch, LANES))
        for k in range(CHUNK // LANES):
            acc = acc + Pc[:, :, k, :]
        for off in (1, 2, 4, 8, 16, 32):
            acc = acc + acc[:, :, lane ^ off]
        tot = acc[:, 0, 0]
        for c in range(1, nch):
            tot = tot + acc[:, c, 0]
        pre = bias + tot
        H[n] = np.where(pre > 0, pre, 0.0)
    return H


def dot(a, b):
    """Products summed in ascending index, left to right."""
    p = a * b
    s = p[0]
    for v in p[1:]:
        s = s + v
    return s


def solve(Hn, Yn, hq, tau=TAU, return_kept=False):
    """The min-norm interpolation with a free intercept through the neighbours (hidden rows Hn
    [m][res], targets Yn [m][d], nearest first) evaluated at hq: modified Gram-Schmidt over
    z_j = h_j - h_0 carrying dy_j = y_j - y_0, rows with |r|^2 <= tau |z_j|^2 dropped;
    pred = y_0, then pred = pred + (q_i . v) * g_i over the kept rows in order."""
    h0, y0 = Hn[0], Yn[0]
    v = hq - h0
    Q, G, kept = [], [], []
    for j in range(1, Hn.shape[0]):
        r = Hn[j] - h0
        g = Yn[j] - y0
        zz = dot(r, r)
        for qi, gi in zip(Q, G):
            c = dot(qi, r)
            r = r - c * qi
            g = g - c * gi
        s = dot(r, r)
        if s > tau * zz:
            sq = np.sqrt(s)
            Q.append(r / sq)
            G.append(g / sq)
            kept.append(j)
    pred = np.array(y0, dtype=np.float64)
    for qi, gi in zip(Q, G):
        pred = pred + dot(qi, v) * gi
    return (pred, kept) if return_kept else pred


def knn(X, q, m):
    """The m nearest rows in (distance, row) order: the oracle's kNN (what nngp_knn computes)."""
    import oracle as O
    return O.knn(X, q, m)[0]


class ElmRef:
    """ELM_base on the contract: fit(x, y, k) keeps the training set and the hidden rows of x
    (computed once per row), predict(new_x) = solve over the m nearest rows."""

    def __init__(self, d, seed=47, res_size=20, R=1, degree=2, m=4, tau=TAU):
        self.d, self.m, self.degree, self.tau = d, m, degree, tau
        self.bias, self.C = draw_weights(d, seed, res_size, degree, R)
        self.x = np.zeros((0, d))
        self.y = np.zeros((0, d))
        self.H = np.zeros((0, res_size))

    def fit(self, x, y, k=0):
        x = np.asarray(x, dtype=np.float64)
        n = self.H.shape[0]
        if x.shape[0] < n or not np.array_equal(x[:n], self.x[:n]):
            n, self.H = 0, self.H[:0]
        self.H = np.vstack([self.H, hidden(x[n:], self.bias, self.C, self.degree)]) if x.shape[0] > n else self.H
        self.x, self.y = x, np.asarray(y, dtype=np.float64)

    def predict(self, new_x, return_kept=False):
        q = np.asarray(new_x, dtype=np.float64).reshape(-1)
        idx = knn(self.x, q, min(self.m, self.x.shape[0]))
        hq = hidden(q, self.bias, self.C, self.degree)[0]
        return solve(self.H[idx], self.y[idx], hq, self.tau, return_kept)


def parareal_elm(system, tspan, N, Ng, Nf, G, F, epsilon=5e-7, u0=None, early_stop=None, **elm):
    """The Parareal loop of oracle.parareal (parareal.py:212-471) with the ELM correction; returns
    dict(t, u, err, k, x, D, converged, conv_int)."""
    import oracle as O
    n = system.d
    order = {'RK1': 1, 'RK2': 2, 'RK4': 4, 'RK8': 8}
    oG, oF = order[G], order[F]
    mdl = ElmRef(n, **elm)
    t = np.linspace(tspan[0], tspan[1], num=N + 1)
    u0 = np.asarray(u0, dtype=float)
    u = np.full((N + 1, n, N + 1), np.nan)
    uG = np.full((N + 1, n, N + 1), np.nan)
    uF = np.full((N + 1, n, N + 1), np.nan)
    err = np.full((N + 1, N), np.nan)
    x = np.zeros((0, n))
    D = np.zeros((0, n))
    conv_int = []
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
        mdl.fit(x, D, k)
        for i in range(I, N):
            uG[i + 1, :, k + 1] = system.rk(oG, t[i], t[i + 1], Ng, u[i, :, k + 1], O.STEP_FIXED)
            u[i + 1, :, k + 1] = mdl.predict(u[i, :, k + 1]) + uG[i + 1, :, k + 1]
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
    return {'t': t, 'u': u[:, :, :k + 1], 'err': err[:, :k + 1], 'k': k + 1, 'x': x, 'D': D,
            'converged': I == N, 'conv_int': conv_int}
