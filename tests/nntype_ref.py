"""CPU restatement of the nntype variants (NNGP_alt, the reference's nnGPara_with_time.py:27-184):
the neighbour selections on the (interval, iteration) table, the prediction on a prescribed list
built from the oracle's parts, and the Parareal loop around them.  Written apart from
nngp_amd.models.NNGP_alt on purpose (iterators and a walked row map here, arithmetic there), so the
two check each other; tests/golden/nntype.npz holds what the reference itself selected.

Cells are (interval, iteration).  `table` is data_x [N][n][>= k+1], NaN where an interval had
converged before that iteration.
"""
from itertools import product

import numpy as np

import oracle as O

NNTYPES = ('nn', 'col+rnd', 'col_only', 'row_col', 'row', 'col_full')
LISTED = NNTYPES[1:]


def filled_cells(table, k):
    """[N][k+1] bool: the cell holds a starting value."""
    return ~np.isnan(np.asarray(table)[:, :, :k + 1]).any(axis=1)


def row_map(filled):
    """{(interval, iteration): training row}: the driver appends each iteration's filled intervals,
    in interval order, as one block."""
    rows, r = {}, 0
    for kk in range(filled.shape[1]):
        for i in range(filled.shape[0]):
            if filled[i, kk]:
                rows[(i, kk)] = r
                r += 1
    return rows


def cycler(i, N):
    """my_cycler(range(i, -1, -1), range(i+1, N)) of the reference, counter included."""
    down, up = iter(range(i, -1, -1)), iter(range(i + 1, N))
    down_out, c = False, 0
    while True:
        v = next(down, None)
        if v is None:
            down_out = True
        else:
            yield v
        v = next(up, None)
        if v is None:
            if down_out:
                break
        else:
            yield v
        if c == 100:
            break
        c += 1


def table_cells(nntype, filled, k, i, nn, stable=True):
    """The cells of the table types in selection order, at most nn (fewer: the reference would fail)."""
    N = filled.shape[0]
    if nntype == 'col_only':
        return [(i, kk) for kk in range(k + 1)]
    if nntype == 'row_col':
        cells = [(ii, kk) for ii in range(N) for kk in range(k + 1)]   # flat index order, interval-major
        cells.sort(key=lambda c: abs(c[1] - k) + abs(c[0] - i))        # list.sort is stable
        seq = iter(cells)
    elif nntype == 'row':
        seq = ((ii, kk) for kk in range(k, -1, -1) for ii in cycler(i, N))
    elif nntype == 'col_full':
        seq = ((ii, kk) for ii in cycler(i, N) for kk in range(k, -1, -1))
    else:
        raise ValueError(nntype)
    out = []
    for c in seq:
        if filled[c]:
            out.append(c)
            if len(out) == nn:
                break
    return out


def neighbour_list(nntype, table, k, i, nn, x=None, rng2=None):
    """The ordered training rows of slice i at iteration k.  col+rnd needs the training inputs x
    [rows][n] and the model's second generator (one permutation is drawn)."""
    filled = filled_cells(table, k)
    rows = row_map(filled)
    if nntype == 'col+rnd':
        c = min(nn, k + 1)
        col = [rows[(i, kk)] for kk in range(k + 1 - c, k + 1)]
        removed = [int(np.argmax(np.any(x == x[r].reshape(1, -1), axis=1))) for r in col]
        cands = rng2.permutation(np.arange(x.shape[0]))[:nn]
        near = [int(r) for r in cands if int(r) not in removed][:nn - c]
        return col + near
    return [rows[c] for c in table_cells(nntype, filled, k, i, k + 1 if nntype == 'col_only' else nn)]


def first_argmin(fv):
    """np.argmin over a scan 'if f < best': a NaN first value wins, later NaNs never, ties keep the first."""
    best = 0
    for t in range(1, len(fv)):
        if fv[t] < fv[best]:
            best = t
    return best


def predict_listed(X, Y, lst, q, theta0, n_restarts=1, fatol=0.1, xatol=0.1, maxfev=400, return_fits=False):
    """The nnGP prediction on the ordered rows lst of (X, Y) at q: oracle.d2_matrix, oracle.nm_fit for
    every (coordinate, jitter, restart) in product order from theta0 [n_fits][2], the first arg-min
    per coordinate and oracle.gp_mean."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    lst = np.asarray(lst, dtype=np.int64)
    xm, ym = np.ascontiguousarray(X[lst]), np.ascontiguousarray(Y[lst])
    d = X.shape[1]
    D2 = O.d2_matrix(xm)
    ins = list(product(range(d), range(len(O.JITTERS)), range(n_restarts)))
    theta0 = np.asarray(theta0, dtype=float).reshape(len(ins), 2)
    fits = np.empty((len(ins), 4))
    for f, (c, j, _) in enumerate(ins):
        th, fv, ne = O.nm_fit(D2, ym[:, c], theta0[f], O.JITTERS[j], fatol, xatol, maxfev)
        fits[f] = (th[0], th[1], fv, ne)
    per = len(O.JITTERS) * n_restarts
    preds = np.empty(d)
    for c in range(d):
        b = c * per + first_argmin(fits[c * per:(c + 1) * per, 2])
        preds[c] = O.gp_mean(xm, ym[:, c], q, fits[b, :2], O.JITTERS[ins[b][1]])
    return (preds, fits) if return_fits else preds


def parareal(system, tspan, N, Ng, Nf, G, F, nntype, nn, epsilon=5e-7, seed=45, u0=None, fatol=0.1, xatol=0.1,
             early_stop=None):
    """oracle.parareal with the NNGP_alt model of one listed nntype: the same loop, the lists from
    neighbour_list on the data_x table.  Returns k, u, conv_int, converged and lists[(k, i)]."""
    assert nntype in LISTED
    n = system.d
    order = {'RK1': 1, 'RK2': 2, 'RK4': 4, 'RK8': 8}
    oG, oF = order[G], order[F]
    t = np.linspace(tspan[0], tspan[1], num=N + 1)
    u0 = np.asarray(u0, dtype=float)
    rng, rng2 = np.random.default_rng(seed), np.random.default_rng(seed)
    u = np.full((N + 1, n, N + 1), np.nan)
    uG = np.full((N + 1, n, N + 1), np.nan)
    uF = np.full((N + 1, n, N + 1), np.nan)
    data_x = np.full((N, n, N), np.nan)
    err = np.full((N + 1, N), np.nan)
    x, D = np.zeros((0, n)), np.zeros((0, n))
    conv_int, lists = [], {}
    u[0] = uG[0] = uF[0] = u0[:, None]
    temp = u0
    for i in range(N):
        temp = system.rk(oG, t[i], t[i + 1], Ng, temp, O.STEP_FIXED)
        uG[i + 1, :, 0] = temp
    u[:, :, 0] = uG[:, :, 0]
    I = 0
    nf = n * len(O.JITTERS)
    for k in range(N):
        uF[I + 1:N + 1, :, k] = system.rk_batch(oF, t[I:N], t[I + 1:N + 1], Nf, u[I:N, :, k], O.STEP_FIXED, 0)
        uG[I + 1, :, k + 1:] = uG[I + 1, :, k].reshape(-1, 1)
        uF[I + 1, :, k + 1:] = uF[I + 1, :, k].reshape(-1, 1)
        u[I + 1, :, k + 1:] = uF[I + 1, :, k].reshape(-1, 1)
        I = I + 1
        x = np.vstack([x, u[I - 1:N, :, k]])
        D = np.vstack([D, uF[I:N + 1, :, k] - uG[I:N + 1, :, k]])
        data_x[I - 1:N, :, k] = u[I - 1:N, :, k]
        if I == N:
            break
        for i in range(I, N):
            uG[i + 1, :, k + 1] = system.rk(oG, t[i], t[i + 1], Ng, u[i, :, k + 1], O.STEP_FIXED)
            lst = neighbour_list(nntype, data_x, k, i, nn, x=x, rng2=rng2)
            lists[(k, i)] = lst
            th0 = rng.integers(-8, 0, (nf, 2)).astype(float)
            preds = predict_listed(x, D, lst, u[i, :, k + 1], th0, 1, fatol, xatol)
            u[i + 1, :, k + 1] = preds + uG[i + 1, :, k + 1]
        err[:, k] = np.linalg.norm(u[:, :, k + 1] - u[:, :, k], np.inf, 1)
        err[I, k] = 0
        for p in range(I + 1, N + 1):
            if err[p, k] < epsilon:
                u[p, :, k + 2:] = u[p, :, k + 1].reshape(-1, 1)
                uG[p, :, k + 2:] = uG[p, :, k + 1].reshape(-1, 1)
                uF[p, :, k + 1:] = uF[p, :, k].reshape(-1, 1)
                I = I + 1
            else:
                break
        conv_int.append(I)
        if I == N or (early_stop is not None and k == early_stop - 1):
            break
    return {'t': t, 'u': u[:, :, :k + 1], 'k': k + 1, 'conv_int': conv_int, 'converged': I == N, 'lists': lists,
            'data_x': data_x[:, :, :k + 1], 'x': x, 'D': D}
