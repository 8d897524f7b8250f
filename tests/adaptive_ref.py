"""Restatement of the adaptive propagator's arithmetic contract: the normative
text of nngp_rk_adaptive (csrc/nngp_rk_adapt.hip) and the bitwise yardstick of
tests/test_gpu_adaptive.py, itself pinned to scipy's solve_ivp by tests/test_adaptive_host.py.

The algorithm is scipy 1.15's RungeKutta._step_impl / rk_step / select_initial_step / norm for the
forward direction, with every sum in a fixed order.  Scalars are Python floats; vectors are NumPy
fp64 arrays used elementwise only (IEEE add, sub, mul, div, abs, maximum: one rounding each, so this
is bit-reproducible).  The two powers are exp(e * log(x)) with the oracle's copies of nngp_math.h's
routines.  Not a test module.

    solve(f, method, t0, t1, nf, u0, rtol, atol, first_step, max_attempts)
        -> (end state, nfev, accepted, rejected, status)

status: 0 reached t1, 1 step size below min_step, 2 max_attempts attempted steps; on 1 and 2 the
state is that of the last accepted step.  One deviation from scipy, where scipy does not end: a NaN
step size is clipped to max_step at the start of a step (scipy keeps it and loops forever)."""
import ctypes
import math

import numpy as np

SAFETY, MIN_FACTOR, MAX_FACTOR = 0.9, 0.2, 10.0

# the published rationals evaluated in double, the same expressions as csrc/nngp_rk_adapt.hip;
# A[s] is row s (entries j < s), E has S + 1 entries (the last one multiplies f_new)
TABLEAUX = {
    'RK23': dict(S=3, err_order=2,   # Bogacki-Shampine 3(2)
                 A=[[], [1.0 / 2], [0.0, 3.0 / 4]],
                 B=[2.0 / 9, 1.0 / 3, 4.0 / 9],
                 E=[5.0 / 72, -1.0 / 12, -1.0 / 9, 1.0 / 8]),
    'RK45': dict(S=6, err_order=4,   # Dormand-Prince 5(4)
                 A=[[], [1.0 / 5], [3.0 / 40, 9.0 / 40], [44.0 / 45, -56.0 / 15, 32.0 / 9],
                    [19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729],
                    [9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656]],
                 B=[35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84],
                 E=[-71.0 / 57600, 0.0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40]),
}
METHOD_CODE = {'RK23': 23, 'RK45': 45}   # enum nngp_adaptive_method


def _oracle_power(x, e):
    """x ** e as nn_exp(e * nn_log(x)), the oracle's copies (orc_exp_array / orc_log_array)"""
    import oracle as O
    L = O.lib()
    a = np.array([x], dtype=np.float64)
    b = np.empty(1)
    dp = ctypes.POINTER(ctypes.c_double)
    L.orc_log_array(1, a.ctypes.data_as(dp), b.ctypes.data_as(dp))
    a[0] = e * float(b[0])
    L.orc_exp_array(1, a.ctypes.data_as(dp), b.ctypes.data_as(dp))
    return float(b[0])


def pymin(*v):
    """Python's min: the first argument unless a later one compares less (a NaN never does)"""
    m = v[0]
    for x in v[1:]:
        if x < m:
            m = x
    return m


def pymax(*v):
    m = v[0]
    for x in v[1:]:
        if x > m:
            m = x
    return m


def tree_sum(x):
    """The contract's sum: column l of 64 is the sequential sum of the elements e = l (mod 64) in
    ascending e, then x[l] += x[l + 32], then 16, ..., 1.  An absent element is +0.0."""
    x = np.asarray(x, dtype=np.float64)
    rows = -(-x.size // 64)
    p = np.zeros(rows * 64)
    p[:x.size] = x
    p = p.reshape(rows, 64)
    col = p[0].copy()
    for r in range(1, rows):
        col = col + p[r]
    w = 32
    while w >= 1:
        col[:w] = col[:w] + col[w:2 * w]
        w //= 2
    return float(col[0])


def rms(x):
    """sqrt(S / d), S the tree sum of the squares"""
    x = np.asarray(x, dtype=np.float64)
    return math.sqrt(tree_sum(x * x) / float(x.size))


def _wsum(coef, K):
    """sum_j coef[j] K[j] over the non-zero coef in ascending j; the first term starts the sum"""
    acc = None
    for c, k in zip(coef, K):
        if c != 0.0:
            v = c * k
            acc = v if acc is None else acc + v
    return acc


def min_step_at(t):
    return 10 * abs(math.nextafter(t, math.inf) - t)


def initial_step(f, y0, f0, interval, max_step, err_order, rtol, atol, power):
    """scipy's select_initial_step (one evaluation of f)"""
    scale = atol + np.abs(y0) * rtol
    d0 = rms(y0 / scale)
    d1 = rms(f0 / scale)
    if d0 < 1e-5 or d1 < 1e-5:
        h0 = 1e-6
    else:
        h0 = 0.01 * d0 / d1
    h0 = pymin(h0, interval)
    y1 = y0 + h0 * f0
    f1 = f(y1)
    d2 = rms((f1 - f0) / scale) / h0
    if d1 <= 1e-15 and d2 <= 1e-15:
        h1 = pymax(1e-6, h0 * 1e-3)
    else:
        h1 = power(0.01 / pymax(d1, d2), 1.0 / (err_order + 1))
    return pymin(100 * h0, h1, interval, max_step)


def solve(f, method, t0, t1, nf, u0, rtol=1e-3, atol=1e-6, first_step=None, max_attempts=None, power=None):
    tab = TABLEAUX[method]
    S, A, B, E = tab['S'], tab['A'], tab['B'], tab['E']
    expo = -1.0 / (tab['err_order'] + 1)
    power = power or _oracle_power
    t0, t1 = float(t0), float(t1)
    if max_attempts is None:
        max_attempts = 100 * nf + 1000
    y = np.array(u0, dtype=np.float64)
    t = t0
    nfev = acc = rej = attempts = 0
    if not t < t1:
        return y, nfev, acc, rej, 0
    interval = t1 - t0
    max_step = interval / float(nf)
    fy = f(y)
    nfev += 1
    if first_step is None:
        h_abs = initial_step(f, y, fy, interval, max_step, tab['err_order'], rtol, atol, power)
        nfev += 1
    else:
        h_abs = float(first_step)
    while True:
        min_step = min_step_at(t)
        if not h_abs <= max_step:      # > max_step, or NaN (the deviation)
            h_abs = max_step
        elif h_abs < min_step:
            h_abs = min_step
        rejected = False
        while True:
            if h_abs < min_step:
                return y, nfev, acc, rej, 1
            if attempts >= max_attempts:
                return y, nfev, acc, rej, 2
            attempts += 1
            t_new = t + h_abs
            if t_new - t1 > 0:
                t_new = t1
            h = t_new - t
            h_abs = abs(h)
            K = [fy]
            for s in range(1, S):
                K.append(f(y + _wsum(A[s], K) * h))
            y_new = y + h * _wsum(B, K)
            f_new = f(y_new)
            K.append(f_new)
            nfev += S
            scale = atol + np.maximum(np.abs(y), np.abs(y_new)) * rtol
            en = rms(_wsum(E, K) * h / scale)
            if en < 1:
                if en == 0:
                    factor = MAX_FACTOR
                else:
                    factor = pymin(MAX_FACTOR, SAFETY * power(en, expo))
                if rejected:
                    factor = pymin(1.0, factor)
                h_abs = h_abs * factor
                break
            h_abs = h_abs * pymax(MIN_FACTOR, SAFETY * power(en, expo))
            rejected = True
            rej += 1
        acc += 1
        t, y, fy = t_new, y_new, f_new
        if not t < t1:
            return y, nfev, acc, rej, 0


def solve_batch(f, method, T0, T1, nf, U0, **kw):
    """solve() per slice: (end states [n][d], stats [n][4] = status, nfev, accepted, rejected)"""
    out = np.empty_like(np.asarray(U0, dtype=np.float64))
    stats = np.zeros((len(out), 4), dtype=np.int64)
    for i in range(len(out)):
        y, nfev, acc, rej, status = solve(f, method, T0[i], T1[i], nf, U0[i], **kw)
        out[i] = y
        stats[i] = (status, nfev, acc, rej)
    return out, stats
