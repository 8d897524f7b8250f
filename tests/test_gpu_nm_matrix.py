"""The GP hyper-parameter fits and the posterior mean pinned to the oracle at every kernel form and
every neighbour count, bitwise.

csrc/nngp_gp.hip, nngp_gpeval.h, nngp_nm.h and nngp_nmlane.hip run a fit padded to one of 8 sizes on
one of about seven kernel forms -- a wave per fit (nm_spec_kernel), two or four waves per fit
(nm_spec2_kernel<M, 2 | 4>), the resume of parked fits (nm_spec2_kernel<M, 0>, or nm_spec_kernel
above 32 neighbours), four fits per wave fused with the arg-min and the mean (nm_fit_kernel<M, true>)
or packed (nm_fit_kernel<M, false>: parking, static or with a work queue), and the lanes kernels at
m = 10 and 15 -- chosen by the fit count against the CU count and six knobs.  tests/nm_cases.py
names knob sets that force each form whatever the card and restates the host dispatch
(tests/test_nm_cases_host.py checks, on the CPU, that the tables below reach every instantiation,
and the oracle against mpmath at the same neighbour counts); here

* nngp_predict -- fits (theta, -LML, nfev), preds and preds + bias -- at every m in 1 .. 64 on the
  one-level, the fused and the parking form, at the smallest and largest m of every padded size on
  every other form, and on both sides of the fused kernel's refusal (n_jitter = 4 / 5 through the
  C ABI above 32 neighbours, where nine jitters never fuse);
* the evaluation caps 1 .. 5 and 9, 10, 11 (below, at and above the park point), tolerance 0 (only
  the iteration rule ends a fit: nfev = maxfev) and tolerance 1e9 (the first check ends every fit
  whose initial simplex spreads less than that: nfev = 3), from starts with zero components;
* nngp_nm_fit_batch on lists that are not in product order, with 1, 9 and 16 jitters, on both sides
  of 4 fits per wave, 16 per workgroup and the work queue's threshold;
* nngp_gp_mean at every m, on both sides of 4 and 16 coordinates per workgroup, with thetas whose
  Cholesky fails or passes on rounding noise alone;
* the 'scale' family: nngp_nm_fit_batch on every form and nngp_gp_mean at every padded size with
  signal variances 10^150.6 .. 10^160 and 10^-151 .. 10^-160 between ordinary ones, so that Cholesky
  pivots leave the range of the short sqrt / reciprocal sequences (in_mid_range) in a wave that
  also holds in-range fits -- the full-sequence branch of nngp_gpeval.h and the k = +-300 rescale of
  sqrt_rcp_exact, which no other input reaches;
* refused arguments, which launch nothing; and nngp_correction_sweep at every padded size (the
  packed batch of the guessed queries, gp_pre_kernel, chain_kernel).

No tolerance anywhere: a form must not change a bit, so all forms of a case share one expectation."""
import ctypes
import functools

import numpy as np
import pytest

import knn_cases as KC
import nm_cases as NC
import oracle as O

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


def _t(torch, a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device='cuda')


def _set_form(monkeypatch, form):
    for k in NC.FORM_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in NC.FORMS[form].items():
        monkeypatch.setenv(k, v)


def _predict_raw(gpu, torch, X, Y, q, m, jit_exp, R, th0, fatol, xatol, maxfev, bias):
    """nngp_predict through the C ABI: (rc, fits, preds, out), the outputs sentinel-filled before."""
    rows, d = X.shape
    n_fits = d * len(jit_exp) * max(R, 1)
    fits = torch.full((max(n_fits, 1), 4), SENTINEL, dtype=torch.float64, device='cuda')
    preds = torch.full((d,), SENTINEL, dtype=torch.float64, device='cuda')
    out = torch.full((d,), SENTINEL, dtype=torch.float64, device='cuda')
    jit, jp = gpu._lib.host_doubles(jit_exp if len(jit_exp) else [0.0])
    Xt, Yt, qt, bt = _t(torch, X), _t(torch, Y), _t(torch, q), _t(torch, bias)
    tt = _t(torch, th0) if th0 is not None else None
    rc = gpu.lib().nngp_predict(Xt.data_ptr(), Yt.data_ptr(), rows, d, qt.data_ptr(), m, len(jit_exp), jp, R,
                                tt.data_ptr() if tt is not None else None, fatol, xatol, maxfev,
                                preds.data_ptr(), bt.data_ptr(), out.data_ptr(), fits.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, fits.cpu().numpy(), preds.cpu().numpy(), out.cpu().numpy()


def _check_predict(gpu, torch, m, variant, d, nj, R, fatol, xatol, maxfev):
    """One prediction case against the oracle's (cached, shared by every form); returns the fits."""
    X, Y, q, th0 = NC.predict_case(m, variant, d, nj, R)
    opreds, ofits = NC.oracle_predict(m, variant, d, nj, R, fatol, xatol, maxfev)
    bias = np.random.default_rng(m + d).standard_normal(d)
    rc, fits, preds, out = _predict_raw(gpu, torch, X, Y, q, m, NC.jitters_for(nj), R, th0, fatol, xatol, maxfev, bias)
    gpu._lib.check(rc)
    assert np.array_equal(fits, ofits, equal_nan=True)
    assert np.array_equal(preds, opreds, equal_nan=True)
    assert np.array_equal(out, opreds + bias, equal_nan=True)
    assert np.all(fits[:, 3] <= maxfev) and np.all(fits[:, 3] >= 1)
    return fits


# ------------------------------------------------------------------------- a. nngp_predict
@pytest.mark.parametrize('row', NC.predict_rows(), ids=NC.predict_row_id)
def test_predict_every_m_and_form_vs_oracle(gpu, row, monkeypatch):
    import torch
    m, variant, form, d, nj, R = row
    if d > 3:
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
        if cus != NC.FUSED_D257_CUS:
            pytest.skip(f'the d = {d} rows are derived for {NC.FUSED_D257_CUS} CUs (two coordinates per '
                        f'workgroup); this card has {cus}')
    _set_form(monkeypatch, form)
    _check_predict(gpu, torch, m, variant, d, nj, R, 0.1, 0.1, 400)


# ----------------------------------------------------------------- b. caps and tolerances
@functools.lru_cache(maxsize=None)
def _first_check_ends(m, variant, nj, R):
    """Fits whose initial simplex spreads at most 1e9 in -LML: scipy's rule ends them at the first
    check (see tests/test_nm_cases_host.py)."""
    X, Y, q, th0 = NC.predict_case(m, variant, 3, nj, R)
    idx, _ = O.knn(X, q, m)
    D2 = O.d2_matrix(X[idx])
    jit = NC.jitters_for(nj)
    out = []
    for f in range(len(th0)):
        c, a = f // (nj * R), (f // R) % nj
        y = np.ascontiguousarray(Y[idx, c])
        ths = [th0[f].copy() for _ in range(3)]
        for k in (0, 1):
            ths[k + 1][k] = 1.05 * th0[f, k] if th0[f, k] != 0 else 0.00025
        fs = np.sort([O.nlml(D2, y, th, jit[a]) for th in ths])
        with np.errstate(invalid='ignore'):
            out.append(bool(np.max(np.abs(fs[0] - fs[1:])) <= 1e9))
    return np.array(out)


@pytest.mark.parametrize('m,variant,form', NC.cap_rows(), ids=lambda v: str(v))
def test_caps_and_tolerances_vs_oracle(gpu, m, variant, form, monkeypatch):
    """maxfev below, at and above the initial simplex, the first iterations and the park point;
    tolerance 0 and 1e9.  The speculative kernels evaluate candidates, and whole later iterations,
    before the state machine asks for them: nfev must still be the oracle's, and never above the cap
    (which holds inside the initial simplex too: maxfev = 1 and 2 end there)."""
    import torch
    _set_form(monkeypatch, form)
    nj, R = NC.form_shape(form, m)
    for tol, maxfev in NC.CAP_SETTINGS:
        fits = _check_predict(gpu, torch, m, variant, 3, nj, R, tol, tol, maxfev)
        if tol == 0.0:
            assert np.all(fits[:, 3] == maxfev)
        if tol == 1e9:
            assert np.array_equal(fits[:, 3] == 3, _first_check_ends(m, variant, nj, R))


# ------------------------------------------------------------------ c. nngp_nm_fit_batch
@functools.lru_cache(maxsize=None)
def _batch_oracle(m, n_fits, nj, fatol, maxfev):
    xm, ym, _ = NC.fit_case(m, NC.BATCH_D)
    coord, jidx, th0 = NC.fit_list(n_fits, NC.BATCH_D, nj, 100 * m + n_fits + nj)
    D2 = O.d2_matrix(xm)
    jit = NC.jitters_for(nj)
    res = [O.nm_fit(D2, ym[:, coord[f]], th0[f], jit[jidx[f]], fatol, fatol, maxfev) for f in range(n_fits)]
    return (np.array([r[0] for r in res]).reshape(n_fits, 2), np.array([r[1] for r in res]),
            np.array([r[2] for r in res], dtype=np.int32))


def _fit_batch_raw(gpu, torch, m, n_fits, nj, fatol, maxfev, want_nfev=True, n_alloc=None):
    xm, ym, _ = NC.fit_case(m, NC.BATCH_D)
    coord, jidx, th0 = NC.fit_list(max(n_fits, 1), NC.BATCH_D, nj, 100 * m + n_fits + nj)
    n_alloc = n_alloc or max(n_fits, 1)
    theta = torch.full((n_alloc, 2), SENTINEL, dtype=torch.float64, device='cuda')
    fval = torch.full((n_alloc,), SENTINEL, dtype=torch.float64, device='cuda')
    nfev = torch.full((n_alloc,), -7, dtype=torch.int32, device='cuda')
    jit, jp = gpu._lib.host_doubles(NC.jitters_for(nj))
    xt, yt, tt = _t(torch, xm), _t(torch, ym), _t(torch, th0)
    ct, jt = _t(torch, coord, torch.int32), _t(torch, jidx, torch.int32)
    rc = gpu.lib().nngp_nm_fit_batch(m, NC.BATCH_D, xt.data_ptr(), yt.data_ptr(), n_fits, ct.data_ptr(), jt.data_ptr(),
                                     nj, jp, tt.data_ptr(), fatol, fatol, maxfev, theta.data_ptr(), fval.data_ptr(),
                                     nfev.data_ptr() if want_nfev else None, None)
    torch.cuda.synchronize()
    return rc, theta.cpu().numpy(), fval.cpu().numpy(), nfev.cpu().numpy()


@pytest.mark.parametrize('m,form', NC.batch_rows(), ids=lambda v: str(v))
def test_fit_batch_shuffled_lists_vs_oracle(gpu, m, form, monkeypatch):
    import torch
    _set_form(monkeypatch, form)
    for nj in NC.BATCH_NJ:
        for n_fits in NC.BATCH_NFITS:
            rc, theta, fval, nfev = _fit_batch_raw(gpu, torch, m, n_fits, nj, 0.1, 400)
            gpu._lib.check(rc)
            oth, ofv, one = _batch_oracle(m, n_fits, nj, 0.1, 400)
            assert np.array_equal(theta, oth) and np.array_equal(fval, ofv, equal_nan=True), (nj, n_fits)
            assert np.array_equal(nfev, one), (nj, n_fits)
    # without nfev_out, and no fits at all
    rc, theta, fval, nfev = _fit_batch_raw(gpu, torch, m, 17, 9, 0.1, 400, want_nfev=False)
    gpu._lib.check(rc)
    oth, ofv, _ = _batch_oracle(m, 17, 9, 0.1, 400)
    assert np.array_equal(theta, oth) and np.array_equal(fval, ofv, equal_nan=True) and np.all(nfev == -7)
    rc, theta, fval, nfev = _fit_batch_raw(gpu, torch, m, 0, 9, 0.1, 400, n_alloc=8)
    assert rc == NC.NNGP_OK
    assert np.all(theta == SENTINEL) and np.all(fval == SENTINEL) and np.all(nfev == -7)


# ------------------------------------------------------------------------ d. nngp_gp_mean
@functools.lru_cache(maxsize=None)
def _mean_case(m, d):
    """(xm, ym, q, theta [d][2], jitter_idx [d], the oracle's means [d]) on the 'dup' set."""
    xm, ym, q = NC.fit_case(m, d)
    rng = np.random.default_rng(64 * d + m)
    theta = rng.integers(-8, 0, (d, 2)).astype(float) + rng.uniform(-0.5, 0.5, (d, 2))
    jidx = ((np.arange(d) * 5 + m) % 9).astype(np.int32)
    hard = (NC.SINGULAR_THETA,) + NC.NEAR_SINGULAR_THETAS
    for i, c in enumerate(range(d // 2, d, 4)):   # singular and nearly singular kernel matrices
        theta[c] = hard[i % len(hard)]
        jidx[c] = i % 3
    want = np.array([O.gp_mean(xm, ym[:, c], q, theta[c], NC.JITTERS[jidx[c]]) for c in range(d)])
    return xm, ym, q, theta, jidx, want


@pytest.mark.parametrize('m', NC.ALL_MS)
def test_gp_mean_every_m_vs_oracle(gpu, m):
    import torch
    jit, jp = gpu._lib.host_doubles(NC.JITTERS)
    nans = 0
    for d in NC.MEAN_D:
        xm, ym, q, theta, jidx, want = _mean_case(m, d)
        out = torch.full((d,), SENTINEL, dtype=torch.float64, device='cuda')
        xt, yt, qt, tt, jt = _t(torch, xm), _t(torch, ym), _t(torch, q), _t(torch, theta), _t(torch, jidx, torch.int32)
        gpu._lib.check(gpu.lib().nngp_gp_mean(m, d, xt.data_ptr(), yt.data_ptr(), qt.data_ptr(), tt.data_ptr(),
                                              jt.data_ptr(), len(jit), jp, out.data_ptr(), None))
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want, equal_nan=True), d
        nans += int(np.isnan(want).sum())
    assert nans >= (1 if m >= 3 else 0)   # (m < 3: the first m rows do not hold the coinciding pair)


# ------------------------------------------------------- d'. pivots outside the mid range
def _scale_fit_batch(gpu, torch, m, fatol, maxfev):
    xm, ym, coord, jidx, th0, _ = NC.scale_fit_case(m)
    n = NC.SCALE_NFITS
    theta = torch.full((n, 2), SENTINEL, dtype=torch.float64, device='cuda')
    fval = torch.full((n,), SENTINEL, dtype=torch.float64, device='cuda')
    nfev = torch.full((n,), -7, dtype=torch.int32, device='cuda')
    jit, jp = gpu._lib.host_doubles(NC.SCALE_JITTERS)
    xt, yt, tt = _t(torch, xm), _t(torch, ym), _t(torch, th0)
    ct, jt = _t(torch, coord, torch.int32), _t(torch, jidx, torch.int32)
    rc = gpu.lib().nngp_nm_fit_batch(m, NC.BATCH_D, xt.data_ptr(), yt.data_ptr(), n, ct.data_ptr(), jt.data_ptr(),
                                     len(jit), jp, tt.data_ptr(), fatol, fatol, maxfev, theta.data_ptr(),
                                     fval.data_ptr(), nfev.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, theta.cpu().numpy(), fval.cpu().numpy(), nfev.cpu().numpy()


@pytest.mark.parametrize('m,form', NC.scale_rows(), ids=lambda v: str(v))
def test_fit_batch_scale_pivots_outside_the_mid_range_vs_oracle(gpu, m, form, monkeypatch):
    """Fits whose pivots lie above 2^500 (1 + 2^-20) or below 2^-500, next to ordinary ones in the
    same wave: nngp_gpeval.h's full sqrt / division branch, taken by the wave-wide ballot, and
    the lanes kernels' 4^+-300 rescale; one matrix crosses the boundary while it is factorised.  The
    caps 3, 9 and 11 end the fits while their simplices are still out of range."""
    import torch
    _set_form(monkeypatch, form)
    for tol, maxfev in NC.SCALE_SETTINGS:
        rc, theta, fval, nfev = _scale_fit_batch(gpu, torch, m, tol, maxfev)
        gpu._lib.check(rc)
        oth, ofv, one = NC.scale_fit_oracle(m, tol, maxfev)
        assert np.array_equal(theta, oth) and np.array_equal(fval, ofv), maxfev
        assert np.array_equal(nfev, one), maxfev


@pytest.mark.parametrize('m', NC.MAXMS)
def test_gp_mean_scale_thetas_vs_oracle(gpu, m):
    """nngp_gp_mean with the same high and low thetas between ordinary ones, at every padded size."""
    import torch
    xm, ym, q, theta, jidx, want, _ = NC.scale_mean_case(m)
    d = NC.SCALE_MEAN_D
    jit, jp = gpu._lib.host_doubles(NC.SCALE_JITTERS)
    out = torch.full((d,), SENTINEL, dtype=torch.float64, device='cuda')
    xt, yt, qt, tt, jt = _t(torch, xm), _t(torch, ym), _t(torch, q), _t(torch, theta), _t(torch, jidx, torch.int32)
    gpu._lib.check(gpu.lib().nngp_gp_mean(m, d, xt.data_ptr(), yt.data_ptr(), qt.data_ptr(), tt.data_ptr(),
                                          jt.data_ptr(), len(jit), jp, out.data_ptr(), None))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


# --------------------------------------------------------------------------- e. refusals
_REFUSALS = {'m=0': dict(m=0), 'm=65': dict(m=65), 'n_jitter=0': dict(nj=0), 'n_jitter=17': dict(nj=NC.MAX_JIT + 1),
             'maxfev=0': dict(maxfev=0), 'n_restarts=0': dict(R=0), 'theta0=NULL': dict(th0=None)}


@pytest.mark.parametrize('what', list(_REFUSALS))
def test_refusals_launch_nothing(gpu, what, monkeypatch):
    """NNGP_E_ARG with the outputs untouched, from nngp_predict and nngp_nm_fit_batch; the next
    valid call is bitwise right."""
    import torch
    bad = _REFUSALS[what]
    X = np.cumsum(0.05 * np.random.default_rng(3).standard_normal((80, 3)), axis=0)
    Y = 0.01 * np.sin(3 * X)
    m, nj, R, maxfev = bad.get('m', 12), bad.get('nj', 9), bad.get('R', 1), bad.get('maxfev', 400)
    th0 = bad.get('th0', np.full((3 * 17 * 2, 2), -3.0))
    rc, fits, preds, out = _predict_raw(gpu, torch, X, Y, X[5] + 0.01, m, NC.jitters_for(nj), R, th0, 0.1, 0.1,
                                        maxfev, np.ones(3))
    assert rc == NC.NNGP_E_ARG and gpu.lib().nngp_last_error()
    assert np.all(fits == SENTINEL) and np.all(preds == SENTINEL) and np.all(out == SENTINEL)
    if 'R' not in bad and 'th0' not in bad and bad.get('m') != 0:
        # (nngp_nm_fit_batch has no restarts; its null theta0 and m = 0 cases need arrays of their own)
        xm, ym = np.ascontiguousarray(X[:64]), np.ascontiguousarray(Y[:64])
        theta = torch.full((4, 2), SENTINEL, dtype=torch.float64, device='cuda')
        fval = torch.full((4,), SENTINEL, dtype=torch.float64, device='cuda')
        nfev = torch.full((4,), -7, dtype=torch.int32, device='cuda')
        z = torch.zeros(4, dtype=torch.int32, device='cuda')
        jit, jp = gpu._lib.host_doubles(NC.jitters_for(nj) if nj else [0.0])
        xt, yt, tt = _t(torch, np.vstack([xm, xm])), _t(torch, np.vstack([ym, ym])), _t(torch, np.full((4, 2), -3.0))
        rc = gpu.lib().nngp_nm_fit_batch(m, 3, xt.data_ptr(), yt.data_ptr(), 4, z.data_ptr(), z.data_ptr(), nj, jp,
                                         tt.data_ptr(), 0.1, 0.1, maxfev, theta.data_ptr(), fval.data_ptr(),
                                         nfev.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == NC.NNGP_E_ARG
        assert bool((theta == SENTINEL).all()) and bool((fval == SENTINEL).all()) and bool((nfev == -7).all())
    _set_form(monkeypatch, 'spec1')
    _check_predict(gpu, torch, 12, 'dup', 3, 9, 1, 0.1, 0.1, 400)


# ----------------------------------------------------------------------------- f. the sweep
def _sweep(gpu, S, speculate):
    """nngp_correction_sweep over the whole case (I = 0): (U1, UG1, spec_hits)."""
    import torch
    ode = gpu.Lorenz(normalization='-11')
    solver = gpu.SolverRK(ode.get_vector_field(), Ng=KC.SWEEP_NG, Nf=KC.SWEEP_NF, F='RK4', G='RK1')
    dev = torch.device('cuda', torch.cuda.current_device())
    cs = solver.f.csystem(dev)
    N, m, d = S['N'], S['m'], 3
    t = _t(torch, S['t'])
    U1 = torch.full((N + 1, d), SENTINEL, dtype=torch.float64, device='cuda')
    UG1 = torch.full((N + 1, d), SENTINEL, dtype=torch.float64, device='cuda')
    U1[0] = _t(torch, S['U1'][0])
    UF, UG, X, Y, th0 = (_t(torch, S[k]) for k in ('UF', 'UG', 'X', 'Y', 'th0'))
    scratch = torch.empty(d, dtype=torch.float64, device='cuda')
    jit, jp = gpu._lib.host_doubles(O.JITTERS)
    hits = ctypes.c_int32(-1)
    gpu._lib.check(gpu.lib().nngp_correction_sweep(
        ctypes.byref(cs), gpu._lib.TABLEAU['RK1'], solver.step_mode, KC.SWEEP_NG, t.data_ptr(), 0, N, U1.data_ptr(),
        UG1.data_ptr(), UF.data_ptr(), UG.data_ptr(), gpu._lib.MODEL_NNGP, X.data_ptr(), Y.data_ptr(), S['rows'], m,
        len(jit), jp, 1, th0.data_ptr(), 0.1, 0.1, 400, scratch.data_ptr(), speculate, ctypes.byref(hits), None,
        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return U1.cpu().numpy(), UG1.cpu().numpy(), int(hits.value)


def _sweep_knobs(m):
    return [None, 'NNGP_HIT_MEAN=0'] + (['NNGP_CHAIN=1'] if m <= NC.CHAIN_MAX_M else [])


@pytest.mark.parametrize('speculate', [0, 1])
@pytest.mark.parametrize('m', NC.SWEEP_MS)
def test_direct_sweep_every_padded_size_vs_oracle_loop(gpu, m, speculate, monkeypatch):
    """U1 and UG1 bitwise the oracle's loop at every padded size, and the predicted hit count with
    re-speculation off; the same with the hit slices' means not precomputed (NNGP_HIT_MEAN=0) and,
    up to m = 24, through the fused chain (NNGP_CHAIN=1)."""
    S = KC.sweep_case('r5000', m)
    assert S['m'] == m
    for knob in _sweep_knobs(m):
        if knob:
            monkeypatch.setenv(*knob.split('='))
        monkeypatch.setenv('NNGP_RESPEC_W', '0')
        U1, UG1, hits = _sweep(gpu, S, speculate)
        assert np.array_equal(U1, S['U1']) and np.array_equal(UG1[1:], S['UG1'][1:]), knob
        assert hits == (sum(S['hit']) if speculate else 0), (knob, hits, S['hit'])
        monkeypatch.delenv('NNGP_RESPEC_W')
        U1w, UG1w, hits_w = _sweep(gpu, S, speculate)   # the default window: gp_pre_kernel for the hits
        assert np.array_equal(U1w, S['U1']) and np.array_equal(UG1w[1:], S['UG1'][1:]), knob
        assert hits_w >= hits if speculate else hits_w == 0
        if knob:
            monkeypatch.delenv(knob.split('=')[0])
