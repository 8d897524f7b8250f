"""CPU: pin the oracle (oracle/nngp_oracle.c + oracle/oracle.py) against fixtures produced by running
the reference itself (tests/golden/gen_golden.py).  No GPU needed.

Tolerances (fp64):
  * ODE right-hand sides and RK end states: bit-exact (same operation order as the reference);
  * PDE right-hand sides: the reference sums dense rows in BLAS order -> |diff| <= 1e-12*max|f|;
  * -LML: relative 1e-6 (ill-conditioned K with jitter 1e-20 amplifies Cholesky order);
  * Nelder-Mead LOGIC: bit-exact vs scipy on the same objective (callback test);
  * end-to-end: same iteration count K where K is roundoff-stable (Parareal, FHN nnGP);
    chaotic Lorenz nnGP: K within +-2 of the reference.
"""
import ctypes
import warnings

import numpy as np
import pytest
from scipy.optimize import minimize

import oracle as O
from conftest import golden
from systems_table import EXACT, KEYS, RK_KEYS, TRIG, oracle_system


@pytest.mark.parametrize('key', KEYS)
def test_rhs_matches_reference(key):
    R = golden('rhs.npz')
    s = oracle_system(key)
    U, F = R[key + '__u'], R[key + '__f']
    out = np.array([s.rhs(u) for u in U])
    if key in EXACT:
        assert np.array_equal(out, F)
    elif key in TRIG:   # fully specified sin/cos vs the reference's libm: a few ulps
        assert np.max(np.abs(out - F)) <= 8 * np.spacing(max(1.0, np.max(np.abs(F))))
    else:
        assert np.max(np.abs(out - F)) <= 1e-12 * max(1.0, np.max(np.abs(F)))


@pytest.mark.parametrize('key', RK_KEYS)
@pytest.mark.parametrize('tab', ['RK1', 'RK2', 'RK4', 'RK8'])
def test_rk_matches_reference(key, tab):
    R = golden('rk.npz')
    s = oracle_system(key)
    k = f'{key}__{tab}'
    u0 = R[k + '__u0']
    t0, t1, steps = R[k + '__span']
    a = s.rk(int(tab[2:]), t0, t1, int(steps), u0, O.STEP_FIXED)
    b = s.rk(int(tab[2:]), t0, t1, int(steps), u0, O.STEP_LINSPACE)
    for got, ref in ((a, R[k + '__fixed']), (b, R[k + '__linspace'])):
        if key in EXACT:
            assert np.array_equal(got, ref)
        else:
            tol = 1e-13 if key in TRIG else 1e-14
            assert np.max(np.abs(got - ref)) <= tol * max(1.0, np.max(np.abs(ref)))


def test_fixed_and_linspace_differ_only_by_roundoff():
    s = oracle_system('lorenz')
    u0 = np.array([-0.8, -0.6, -0.3])
    a = s.rk(4, 0.0, 1.7, 37, u0, O.STEP_FIXED)
    b = s.rk(4, 0.0, 1.7, 37, u0, O.STEP_LINSPACE)
    assert np.max(np.abs(a - b)) < 1e-12


@pytest.mark.parametrize('tag', ['paged', 'paged73'])
def test_paging_quirk_matches_reference(tag):
    R = golden('rk.npz')
    s = oracle_system('lorenz')
    t0, t1, steps, thresh = R[tag + '__lorenz__args']
    thresh = thresh if tag == 'paged73' else int(thresh)
    out = O.paged(lambda a, b, st, u: s.rk(4, a, b, st, u), t0, t1, int(steps), thresh, R['paged__lorenz__u0'])
    assert np.array_equal(out, R[tag + '__lorenz__out'])


def test_global_grid_is_the_linspace_grid():
    s = oracle_system('lorenz')
    u0 = np.array([-0.8, -0.6, -0.3])
    whole = s.rk(1, 0.0, 0.37, 64, u0, O.STEP_LINSPACE)
    x = u0
    for i in range(8):
        x = s.rk_grid(1, 0.0, 0.37, 64, 8 * i, 8, x)
    assert np.all(np.isfinite(whole)) and np.array_equal(x, whole)


def test_math_accuracy():
    """The shared exp / log / 10^x / sin / cos (GPU csrc/nngp_math.h == oracle) stay within 2 ulp of glibc."""
    L = O.lib()
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.uniform(-745, 709, 20000), rng.uniform(-1, 1, 20000), [0.0, -0.0, 1e-300]])
    got = np.array([L.nn_exp(x) for x in xs])
    ref = np.exp(xs)
    ok = np.isfinite(ref) & (ref > 1e-300)
    assert np.max(np.abs(got[ok] - ref[ok]) / np.spacing(ref[ok])) <= 2
    assert L.nn_exp(800.0) == np.inf and L.nn_exp(-800.0) == 0.0 and np.isnan(L.nn_exp(np.nan))
    ps = rng.uniform(-300, 300, 20000)
    got = np.array([L.nn_pow10(x) for x in ps])
    ref = 10.0 ** ps
    assert np.max(np.abs(got - ref) / np.spacing(ref)) <= 2
    ls = np.exp(rng.uniform(-700, 700, 20000))
    got = np.array([L.nn_log(x) for x in ls])
    assert np.max(np.abs(got - np.log(ls)) / np.spacing(np.abs(np.log(ls)))) <= 2
    assert L.nn_log(0.0) == -np.inf and np.isnan(L.nn_log(-1.0))
    xs = np.concatenate([rng.uniform(-40, 40, 20000), rng.uniform(-1e4, 1e4, 2000), [0.0, np.pi / 2, -np.pi]])
    for fn, ref in (('nn_sin', np.sin), ('nn_cos', np.cos), ('nn_sin_pi', np.sin)):
        got = np.array([getattr(L, fn)(x) for x in xs])
        r = ref(xs)
        assert np.max(np.abs(got - r) / np.maximum(np.spacing(np.abs(r)), np.spacing(1.0) * 2 ** -10)) <= 2, fn
    assert np.isnan(L.nn_sin(np.inf)) and np.isnan(L.nn_cos(np.nan))
    assert np.isnan(L.nn_sin_pi(np.inf)) and np.isnan(L.nn_sin_pi(-np.inf)) and np.isnan(L.nn_sin_pi(np.nan))
    # the pi-reduced sine at 200k points covering ThomasLabyrinth's attractor bound |x| <= b/a = 20
    # (systems.py:257-271, a = 0.5, b = 10) with margin, and at +-0
    xs = np.concatenate([rng.uniform(-25, 25, 200000), [20.0, -20.0, 25.0, -25.0]])
    got = np.array([L.nn_sin_pi(x) for x in xs])
    assert np.max(np.abs(got - np.sin(xs)) / np.maximum(np.spacing(np.abs(np.sin(xs))), 2.0 ** -1074)) <= 2
    assert L.nn_sin_pi(0.0) == 0.0 and L.nn_sin_pi(1e-300) == 1e-300   # (the sign of a zero is not kept)


def _true_error_ulps(mp, got, true, floor_exp=-1074):
    """max over the points of |got - true| / ulp(true), with ulp(true) = 2^(e - 53) for
    2^(e-1) <= |true| < 2^e and never below 2^floor_exp; and the index of the worst point."""
    worst, at = 0.0, -1
    for i, (g, t) in enumerate(zip(got, true)):
        e = mp.frexp(t)[1] if t != 0 else floor_exp
        err = float(mp.ldexp(abs(mp.mpf(float(g)) - t), -max(e - 53, floor_exp)))
        if not err <= worst:
            worst, at = err, i
    return worst, at


def test_math_true_error():
    """The oracle's exp / 10^x / log / sin / cos against the true values (mpmath, 200 bits), in ulps
    of the true value, on fixed-seed sets of 20 000 points per function.  exp, 10^x and log stay
    within 1 ulp -- subnormal results included, where an ulp is 2^-1074 -- and the three sines and
    cosines within 2 ulp on |x| <= 1e4, with the absolute floor max(ulp(true), 2^-62) of
    test_math_accuracy: next to a multiple of pi the error of the three-term reduction, ~1e-26 in
    absolute terms, is many ulps of a tiny true value (x = RN(29 pi): sin(x) = 5.3e-15 with an
    absolute error of 5e-27, i.e. 2.6e4 ulp of it, and harmless for a vector field).  Measured:
        nn_exp, x in [-708, 709] and [-1, 1]      0.81       nn_sin / nn_cos, |x| <= 1e4   1.78 / 1.58
        nn_exp, subnormal results                 0.80       nn_sin_pi, |x| <= 25          1.35
        nn_pow10, x in [-307, 308]                0.93       nn_sin_pi, |x| <= 1e4         1.78
        nn_log                                    0.62       nn_sin / nn_cos, |x| <= 1e5   2.23 / 1.96
    (the |x| <= 1e5 figures are recorded, under the next whole ulp, 3; csrc/nngp_math.h and DESIGN.md
    quote all of them).
    tests/test_gpu_math_probe.py pins the device's copy to this one bit for bit on the same
    domains, so the bounds hold for the device too."""
    mp = pytest.importorskip('mpmath').mp
    mp.prec = 200
    L = O.lib()
    rng = np.random.default_rng(20)
    N = 20000
    f1 = lambda name, xs: np.array([getattr(L, name)(float(x)) for x in xs])
    report = {}

    def check(label, name, xs, truth, bound, floor_exp=-1074):
        got = f1(name, xs)
        assert np.isfinite(got).all(), label
        worst, at = _true_error_ulps(mp, got, [truth(mp.mpf(float(x))) for x in xs], floor_exp)
        report[label] = worst
        print(f'{label}: worst true error {worst:.3f} ulp at x = {float(xs[at])!r} ({float(xs[at]).hex()})')
        assert worst <= bound, (label, worst, float(xs[at]).hex())

    check('nn_exp', 'nn_exp', np.concatenate([rng.uniform(-708, 709, N // 2), rng.uniform(-1, 1, N // 2)]), mp.exp, 1.0)
    check('nn_exp, subnormal results', 'nn_exp', rng.uniform(-745.13, -708.4, N), mp.exp, 1.0)
    check('nn_pow10', 'nn_pow10', rng.uniform(-307, 308, N), lambda x: mp.power(10, x), 1.0)
    check('nn_log', 'nn_log', np.exp(rng.uniform(-745, 709, N)), mp.log, 1.0)
    x4, x25, x5 = rng.uniform(-1e4, 1e4, N), rng.uniform(-25, 25, N), rng.uniform(-1e5, 1e5, N)
    check('nn_sin, |x| <= 1e4', 'nn_sin', x4, mp.sin, 2.0, -62)
    check('nn_cos, |x| <= 1e4', 'nn_cos', x4, mp.cos, 2.0, -62)
    check('nn_sin_pi, |x| <= 25', 'nn_sin_pi', x25, mp.sin, 2.0, -62)
    check('nn_sin_pi, |x| <= 1e4', 'nn_sin_pi', x4, mp.sin, 2.0, -62)
    # beyond the bound's range: recorded, not promised (n PIO2_3's rounding grows with |n|)
    check('nn_sin, |x| <= 1e5', 'nn_sin', x5, mp.sin, 3.0, -62)
    check('nn_cos, |x| <= 1e5', 'nn_cos', x5, mp.cos, 3.0, -62)
    # the example of the floor: relative to the tiny true value the error is tens of thousands of ulp
    x29 = -91.106186954104
    t = mp.sin(mp.mpf(x29))
    rel = float(abs(mp.mpf(L.nn_sin(x29)) - t) / mp.ldexp(1, mp.frexp(t)[1] - 53))
    assert abs(float(t)) < 1e-14 and rel > 1e3 and float(abs(mp.mpf(L.nn_sin(x29)) - t)) < 2.0 ** -62
    mp.prec = 53


def test_nlml_matches_reference():
    L = golden('lml.npz')
    D2 = O.d2_matrix(L['xm'])
    v = np.array([[[O.nlml(D2, L['ym'][:, j], th, jit) for j in range(3)] for th in L['thetas']]
                  for jit in L['jitters']])
    ref = L['nlml']
    assert np.array_equal(np.isinf(v), np.isinf(ref))
    both = np.isfinite(v) & np.isfinite(ref)
    rel = np.abs(v[both] - ref[both]) / np.maximum(1, np.abs(ref[both]))
    print(f'-LML vs the reference over {both.sum()} finite points: bitwise {np.mean(v[both] == ref[both]):.3f}, '
          f'relative error median {np.median(rel):.2e}, 99th percentile {np.quantile(rel, 0.99):.2e}, max {rel.max():.2e}')
    # measured: bitwise 0.343, median 1.8e-16, p99 1.5e-7, max 4.1e-7 -- the large
    # ones at -LML ~ 2e10, kernels so ill-conditioned (jitter 1e-20) that cond(K) * 1e-16 is ~1e-7
    assert np.mean(v[both] == ref[both]) >= 0.30
    assert rel.max() < 1e-6 and np.quantile(rel, 0.99) < 5e-7
    assert np.median(rel) < 1e-15


def test_nlml_singular_kernel_failure_semantics():
    """Duplicated rows: K is singular without jitter; a failed Cholesky is +inf (models.py:250)."""
    L = golden('lml.npz')
    D2 = O.d2_matrix(L['xd'])
    v = np.array([[O.nlml(D2, L['yd'][:, 0], th, jit) for th in L['thetas']] for jit in L['jitters']])
    ref = L['nlml_dup']
    agree = (np.isinf(v) == np.isinf(ref)).mean()
    print(f'Cholesky pass/fail vs the reference on duplicated rows: {agree:.4f} '
          f'({(np.isinf(v) != np.isinf(ref)).sum()} flips of {v.size})')
    # measured: 2 flips of 1089 (0.9982), both at the numerical edge of positive-definiteness
    assert agree >= 0.997
    both = np.isfinite(v) & np.isfinite(ref)
    rel = np.abs(v[both] - ref[both]) / np.maximum(1, np.abs(ref[both]))
    assert np.median(rel) < 1e-10


def test_posterior_mean_matches_reference():
    L = golden('lml.npz')
    pm = np.array([[O.gp_mean(L['xm'], L['ym'][:, j], L['new_x'], th, -15.0) for j in range(3)]
                   for th in L['thetas']])
    ref = L['post_mean_jit15']
    assert np.array_equal(np.isnan(pm), np.isnan(ref))
    assert np.nanmax(np.abs(pm - ref)) < 1e-8


# --------------------------------------------------------------------------------------------
# Nelder-Mead: the C restatement vs scipy on the SAME objective -> bit-exact
# --------------------------------------------------------------------------------------------
_CB = ctypes.CFUNCTYPE(ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p)


def _c_nm(fn, th0, fatol, xatol, maxfev):
    L = O.lib()
    L.orc_nm_core.argtypes = [_CB, ctypes.c_void_p, O._dp, ctypes.c_double, ctypes.c_double, ctypes.c_int,
                              O._dp, O._dp, ctypes.POINTER(ctypes.c_int)]
    cb = _CB(lambda x, ctx: float(fn(np.array([x[0], x[1]]))))
    th0 = np.ascontiguousarray(th0, dtype=float)
    th = np.empty(2)
    fv = np.empty(1)
    ne = ctypes.c_int()
    L.orc_nm_core(cb, None, O._p(th0), fatol, xatol, maxfev, O._p(th), O._p(fv), ctypes.byref(ne))
    return th, fv[0], ne.value


def _objectives():
    L = golden('nm.npz')
    xm, ym = L['m10__xm'], L['m10__ym']
    D2 = O.d2_matrix(xm)
    yield 'lml', lambda th: O.nlml(D2, ym[:, 0], th, -15.0)
    yield 'lml_jit20', lambda th: O.nlml(D2, ym[:, 2], th, -20.0)
    yield 'rosen', lambda th: (1 - th[0]) ** 2 + 100 * (th[1] - th[0] ** 2) ** 2
    yield 'inf_region', lambda th: np.inf if th[0] + th[1] > -3 else (th[0] + 2) ** 2 + (th[1] + 4) ** 4
    yield 'flat', lambda th: 1.0


@pytest.mark.parametrize('maxfev', [400, 7, 12])
def test_nelder_mead_logic_bit_exact_vs_scipy(maxfev):
    rng = np.random.default_rng(0)
    for name, fn in _objectives():
        for _ in range(6):
            th0 = rng.integers(-8, 0, 2).astype(float)
            for tol in (0.1, 1e-3):
                ref = minimize(fn, th0, method='Nelder-Mead',
                               options={'fatol': tol, 'xatol': tol, 'maxfev': maxfev, 'maxiter': maxfev})
                th, fv, ne = _c_nm(fn, th0, tol, tol, maxfev)
                assert ne == ref.nfev, name
                assert np.array_equal(th, ref.x), name
                assert fv == ref.fun or (np.isinf(fv) and np.isinf(ref.fun)), name


@pytest.mark.parametrize('maxfev', [1, 2, 3, 4, 5, 6, 9, 10, 11, 400])
def test_nelder_mead_caps_zero_starts_and_tolerance_edges_vs_scipy(maxfev):
    """The same at the evaluation caps around the initial simplex and the first iterations, from
    starts with zero components (the 0.00025 branch of the initial simplex), with tolerance 0 (only
    the iteration rule ends the fit) and 1e9 (the first check ends it)."""
    rng = np.random.default_rng(1)
    for name, fn in _objectives():
        for zero in ((0,), (1,), (0, 1), ()):
            th0 = rng.integers(-8, 0, 2).astype(float)
            th0[list(zero)] = 0.0
            for tol in (0.0, 0.1, 1e9):
                if maxfev == 400 and tol == 0.0 and name != 'flat':
                    continue   # (400 evaluations of a python callback per case; 'flat' keeps the cap)
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore')
                    ref = minimize(fn, th0, method='Nelder-Mead',
                                   options={'fatol': tol, 'xatol': tol, 'maxfev': maxfev, 'maxiter': maxfev})
                th, fv, ne = _c_nm(fn, th0, tol, tol, maxfev)
                assert ne == ref.nfev <= max(maxfev, 1), (name, zero, tol)
                assert np.array_equal(th, ref.x), (name, zero, tol)
                assert fv == ref.fun or (np.isinf(fv) and np.isinf(ref.fun)), (name, zero, tol)


def test_nm_fits_track_reference():
    """Full fits on the reference -LML.  Per-fit iterates are NOT bitwise the reference's: the
    oracle's exp / 10^x / log and its sum orders differ from numpy's in the last ulp, which
    redirects Nelder-Mead in flat directions (tools/fit_agreement.py attributes every mismatch:
    profiles/r05/fit_agreement.txt); the optimum value agrees.  Measured: 80 of 81
    optimum values within 1e-6, 21 of 81 fits bitwise."""
    N = golden('nm.npz')
    agree, bitwise = [], []
    for tag in ['m10', 'm18tol3', 'm30']:
        xm, ym, ins, th0, tol, out = [N[tag + '__' + k] for k in ['xm', 'ym', 'ins', 'th0', 'tol', 'out']]
        D2 = O.d2_matrix(xm)
        for q, (j, jit) in enumerate(ins):
            th, fv, ne = O.nm_fit(D2, ym[:, int(j)], th0[q], jit, tol[0], tol[1])
            agree.append(abs(fv - out[q, 2]) <= 1e-6 * max(1, abs(out[q, 2])))
            bitwise.append(np.array_equal(th, out[q, :2]) and fv == out[q, 2])
    print(f'NM fits vs the reference: optimum within 1e-6 {sum(agree)}/{len(agree)}, '
          f'bitwise {sum(bitwise)}/{len(bitwise)}')
    assert sum(agree) >= len(agree) - 3 and sum(bitwise) >= 15


def test_knn_matches_reference_up_to_exact_ties():
    K = golden('knn.npz')
    idx, dist = O.knn(K['X'], K['q'], K['X'].shape[0])   # full ordering, incl. the 7/100 tie
    ref = K['idx']
    assert np.array_equal(dist, K['dist'][ref])          # same distances, same order
    for a, b in zip(idx, ref):
        assert a == b or K['dist'][a] == K['dist'][b]     # only exact ties may permute
    assert idx[list(idx).index(7)] == 7 and (100 in idx)  # tie broken by row index (7 before 100)
    assert list(idx).index(7) < list(idx).index(100)


def test_predict_d128_matches_reference():
    """One NNGP_p.predict at d=128, m=15 (1152 fits) on Parareal-like data."""
    P = golden('preds_d128.npz')
    rng = np.random.default_rng(int(P['seed']))
    th0 = rng.integers(-8, 0, (1152, 2)).astype(float)
    assert np.array_equal(th0, P['rnd'])                  # the reference's draw order (models.py:192)
    idx, _ = O.knn(P['X'], P['new_x'], int(P['m']))
    assert np.array_equal(P['X'][idx], P['xm'])           # same neighbours, same order
    preds, fits = O.predict(P['X'], P['Y'], P['new_x'], int(P['m']), th0, return_fits=True)
    ref = P['preds']
    scale = np.max(np.abs(ref))
    close = np.abs(preds - ref) <= 1e-8 * scale
    r = P['fit_res']
    fclose = np.abs(fits[:, 2] - r[:, 2]) <= 1e-6 * np.maximum(1, np.abs(r[:, 2]))
    print(f'predictions within 1e-8 of scale: {close.sum()}/128, max {np.max(np.abs(preds - ref)) / scale:.2e} of '
          f'scale; fit optima within 1e-6: {fclose.sum()}/1152')
    # measured (profiles/r05/fit_agreement.txt): 127 of 128 predictions within 1e-8 of the scale,
    # the other (coordinate 5: the same arg-min jitter, an optimum elsewhere inside the 0.1
    # tolerance) 2.0e-5 of it; 1 096 of 1 152 optima within 1e-6 -- the other 56 are fits that
    # stopped elsewhere inside xatol / fatol = 0.1 after an ulp-level difference in exp / 10^x
    # (53 % of all path differences) or in log and the sum orders (44 %)
    assert close.sum() >= 126 and np.max(np.abs(preds - ref)) <= 1e-4 * scale
    assert fclose.sum() >= 1070


# --------------------------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------------------------
def test_parareal_lorenz_matches_reference():
    """BASELINE configs[0] (Lorenz N=32, G=F=RK4 6/450 steps per slice): Parareal K and iterates."""
    P = golden('para_lorenz.npz')
    s = O.System('lorenz')
    r = O.parareal(s, [0, 18], 32, 6, 450, 'RK4', 'RK4', model='parareal', u0=s.fit([-15, -15, 20]))
    assert r['k'] == int(P['para__k'])
    assert r['conv_int'] == list(P['para__conv_int'])
    assert np.nanmax(np.abs(r['u'] - P['para__u'])) < 1e-9


def test_nngp_lorenz_seed_k_within_chaos_spread():
    P = golden('para_lorenz.npz')
    s = O.System('lorenz')
    ks = []
    for seed in (45, 47):
        r = O.parareal(s, [0, 18], 32, 6, 450, 'RK4', 'RK4', model='nngp', nn=10, seed=seed,
                       u0=s.fit([-15, -15, 20]))
        ks.append(r['k'])
        assert abs(r['k'] - int(P[f'nngp_s{seed}__k'])) <= 2
        assert r['converged']


def test_fhn_ode_parareal_and_nngp_match_reference():
    P = golden('para_fhn.npz')
    s = O.System('fhn_ode')
    u0 = s.fit([-1, 1])
    r = O.parareal(s, [0, 40], 40, 4, 4000, 'RK2', 'RK4', model='parareal', u0=u0)
    assert r['k'] == int(P['para__k'])
    assert np.nanmax(np.abs(r['u'] - P['para__u'])) < 1e-9
    r = O.parareal(s, [0, 40], 40, 4, 4000, 'RK2', 'RK4', model='nngp', nn=15, seed=45, u0=u0)
    assert r['k'] == int(P['nngp_s45__k'])
    assert r['conv_int'] == list(P['nngp_s45__conv_int'])
    # intermediate iterates carry GP roundoff (NM branch flips); the converged column does not
    assert np.nanmax(np.abs(r['u'] - P['nngp_s45__u'])) < 1e-3
    assert np.max(np.abs(r['u'][:, :, -1] - P['nngp_s45__u'][:, :, -1])) < 5e-7   # eps


# ---------------------------------------------------------------- full-data GParareal (GPjax_p)
def test_gp_oracle_fits_match_reference():
    """oracle/gpfull.py restates GPjax_p's -LML + Nelder-Mead (models.py:306-335); on the
    reference's own recorded training fan-outs (gen_golden.py part_gp) every fit agrees."""
    import gpfull as GF
    P = golden('gp_lorenz.npz')
    for c in (0, 1):
        x, y, old, tol = P[f'call{c}__x'], P[f'call{c}__y'], P[f'call{c}__old'], P[f'call{c}__tol']
        for (j, jit), ref in zip(P[f'call{c}__ins'], P[f'call{c}__res']):
            th, fv, _ = GF.gp_fit(x, y[:, int(j)], old[int(j)], jit, tol[0], tol[1])
            np.testing.assert_allclose(th, ref[:2], rtol=1e-12, atol=0)
            assert fv == pytest.approx(ref[2], rel=1e-12) or (np.isinf(fv) and np.isinf(ref[2]))


def test_gp_oracle_lml_matches_reference():
    import gpfull as GF
    P = golden('gp_lorenz.npz')
    x, y = P['call1__x'], P['call1__y']
    for j, (th, jit, ref) in enumerate(zip(P['lml_theta'], P['lml_jitter'], P['lml_val'])):
        v = GF.gp_nlml(x, y[:, j % 3], th, jit)
        assert v == pytest.approx(ref, rel=1e-12) or (np.isinf(v) and np.isinf(ref))


@pytest.mark.parametrize('case', ['burgers', 'fhn_pde'])
def test_dense_reference_formulation_equals_stencil(case):
    """The CPU baseline's "reference formulation" (the reference's dense Dxx@u / (a L)@u1
    matrices, systems.py:321-446, every entry multiplied, each row summed over columns in
    ascending order) gives the stencil oracle's RK trajectories bit for bit -- only the cost
    differs (d^2 per matvec)."""
    if case == 'burgers':
        st = O.System('burgers', d=128, param=(0.01,), mn=0.0, mx=1.0)
        dn = O.System('burgers', d=128, param=(0.01,), mn=0.0, mx=1.0, dense=True)
        x = np.linspace(-1, 1, 128)
        u0 = st.fit(0.5 * (np.cos(4.5 * np.pi * x) + 1))
        T, steps = 5.0 / 128, 200
    else:
        st = O.System('fhn_pde', nx=10, mn=-1, mx=1)
        dn = O.System('fhn_pde', nx=10, mn=-1, mx=1, dense=True)
        u0 = np.random.default_rng(45).uniform(-1, 1, 200)
        T, steps = 0.05, 50
    U = np.stack([u0, 0.9 * u0, u0[::-1].copy()])
    t0, t1 = np.array([0.0, T, 2 * T]), np.array([T, 2 * T, 3 * T])
    for mode in (O.STEP_FIXED, O.STEP_LINSPACE):
        a = st.rk_batch(8, t0, t1, steps, U, mode)
        b = dn.rk_batch(8, t0, t1, steps, U, mode)
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)


def test_cholesky_pass_fail_follows_lapack_on_duplicated_neighbours():
    """The -LML's pass/fail bit on near-singular kernels steers Nelder-Mead (a spurious pass gives
    a hugely negative -LML that wins the arg-min; models.py:207-217).  The reference factors with
    LAPACK dpotrf (jax -> OpenBLAS dpotf2 for these sizes), so the oracle (and the HIP kernel, bit
    for bit) sums in dpotf2's order.  Against numpy's LAPACK on exactly duplicated rows (K =
    psy*ones + jitter*I, the jitter often below psy*2^-53: FHN-PDE's steady state) and on clusters
    of near-duplicates, pass/fail must agree on >= 99 % (round 1's successive subtraction: 89 %)."""
    rng = np.random.default_rng(11)
    agree, total, false_pass = 0, 0, 0
    for t in range(1500):
        if t % 2 == 0:
            m = int(rng.choice([10, 15, 20, 24]))
            xm = np.tile(rng.standard_normal((1, 3)), (m, 1))
        else:
            m = int(rng.choice([15, 20]))
            c = int(rng.integers(1, 5))
            base = rng.standard_normal((c, 3))
            xm = base[rng.integers(0, c, m)] + 10 ** rng.uniform(-12, -4) * rng.standard_normal((m, 3))
        D2 = O.d2_matrix(xm)
        th = (rng.uniform(-8, 0), rng.uniform(-4, 1))
        jit = float(rng.integers(-20, -11))
        K = 10 ** th[1] * np.exp(-0.5 * (1 / 10 ** th[0]) * D2)
        K[np.diag_indices(m)] += 10.0 ** jit
        try:
            np.linalg.cholesky(K)
            ref_ok = True
        except np.linalg.LinAlgError:
            ref_ok = False
        ours_ok = np.isfinite(O.nlml(D2, np.zeros(m) + 1e-3, th, jit))
        agree += ref_ok == ours_ok
        false_pass += ours_ok and not ref_ok
        total += 1
    assert agree / total >= 0.99, agree / total
    assert false_pass / total <= 0.01
