"""Shared inputs of tests/test_nm_cases_host.py (CPU) and tests/test_gpu_nm_matrix.py (GPU): seeded
case recipes for the GP hyper-parameter fits and the posterior mean, the named knob sets that force
one kernel form of csrc/nngp_gp.hip / csrc/nngp_nmlane.hip whatever the CU count, and a Python
restatement of the host dispatch under those knobs (use_spec, spec_waves, run_nm_spec, run_nm,
run_nm_parked, run_nm_lanes) that says which kernel template a call reaches.

The fits run padded to one of 8 sizes (maxm_for) and the arithmetic order of one evaluation depends
on the exact m (dpotf2's (m-1-j) & 3 tail rows, the lane pairing (l, l+16), GP<M>::tail_set), so
the tables are per m, not per padded size.  The 'scale' family holds fits and means whose Cholesky
pivots leave the range of the short sqrt / reciprocal sequences.  No GPU is needed to build a case."""
import functools

import numpy as np

# ------------------------------------------------------------------- the padded sizes, restated
MAXMS = (8, 16, 18, 20, 24, 32, 48, 64)   # csrc/nngp_gp.hip maxm_for
MAX_M = 64
MAX_JIT = 16                              # csrc/nngp_nmargs.h
LANE_MS = (10, 15)                        # csrc/nngp_nmlane.hip with_lane_m
CHAIN_MAX_M = 24                          # csrc/nngp_gp.hip chain_supported
NNGP_OK, NNGP_E_ARG = 0, -1               # include/nngp.h


def maxm_for(m):
    return next(M for M in MAXMS if m <= M)


def gp_mmin(maxm):
    """csrc/nngp_gpeval.h gp_mmin: the smallest m a padded size serves."""
    i = MAXMS.index(maxm)
    return 1 if i == 0 else MAXMS[i - 1] + 1


# the smallest and the largest m of every padded size
EDGE_MS = sorted({gp_mmin(M) for M in MAXMS} | set(MAXMS))
ALL_MS = list(range(1, MAX_M + 1))


def k_image_doubles(maxm):
    """GP<MAXM>::IMG: the K/L image and the four per-row scalars of one fit, in doubles."""
    rpl = (maxm + 15) // 16
    xoff = 8 * rpl * (16 * rpl + 1) if maxm > 32 else maxm * (maxm + 1)
    return xoff + 4 * maxm


def nm_tmax(maxm):
    """NMBound<MAXM>::T: the launch bound of nm_fit_kernel."""
    return 512 if maxm <= 16 else (256 if maxm <= 32 else 64)


# ------------------------------------------------------------------------------- case recipes
JITTERS = np.arange(-20, -11, dtype=float)
VARIANTS = ('smooth', 'dup', 'zero')


def jitters_for(n_jitter):
    """The n_jitter exponents ending at -12 (n_jitter = 9: the reference's -20 .. -12)."""
    return np.arange(-11 - n_jitter, -11, dtype=float)


def predict_case(m, variant, d=3, n_jitter=9, R=1):
    """(X [m+7][d], Y, q [d], theta0 [d*n_jitter*R][2]) of one prediction with m neighbours.
    'dup': two of the neighbours coincide (Y keeps every row's own value), so the low-jitter kernel
    matrices are singular, simplices mix +inf and finite vertices and some fits run to the cap.
    'zero': 'smooth' with zero components in theta0, the 0.00025 branch of the initial simplex."""
    assert variant in VARIANTS
    rng = np.random.default_rng((2000 if variant == 'dup' else 1000) + m)
    X = np.cumsum(0.05 * rng.standard_normal((m + 7, d)), axis=0)
    Y = 0.01 * np.sin(3 * X) + 1e-5 * rng.standard_normal(X.shape)
    q = X[m // 2] + 0.01
    theta0 = rng.integers(-8, 0, (d * n_jitter * R, 2)).astype(float)
    if variant == 'dup' and m >= 2:
        X[m // 2 + 1] = X[m // 2]
    if variant == 'zero':
        theta0[::2, 0] = 0
        theta0[1::3, 1] = 0
    return X, Y, q, theta0


def fit_case(m, d, variant='dup'):
    """(xm [m][d], ym [m][d]) for nngp_nm_fit_batch / nngp_gp_mean: the first m rows of the
    prediction case (for 'dup' and m >= 3 they hold the coinciding pair) and its query."""
    X, Y, q, _ = predict_case(m, variant, d)
    return np.ascontiguousarray(X[:m]), np.ascontiguousarray(Y[:m]), q


def fit_list(n_fits, d, n_jitter, seed):
    """(coord, jitter_idx, theta0) of n_fits fits: shuffled coordinates with repeats and random
    jitter indices -- not the product(coord, jitter) order of a prediction."""
    rng = np.random.default_rng(seed)
    coord = rng.integers(0, d, n_fits).astype(np.int32)
    jidx = rng.integers(0, n_jitter, n_fits).astype(np.int32)
    theta0 = rng.integers(-8, 0, (n_fits, 2)).astype(float)
    return coord, jidx, theta0


# -------------------------------------------------------------------------------------- forms
_PACKED = {'NNGP_NM_SPEC': '0', 'NNGP_NM_PARK': '0'}
PARK_CAP = 10   # the park forms hand a fit over at 10 evaluations
_PARK = {'NNGP_NM_SPEC': '0', 'NNGP_NM_PARK': str(PARK_CAP)}
# (the lanes kernels sit behind run_nm_parked, so they too need the speculative kernel off)
FORMS = {
    'spec1': {'NNGP_NM_SPEC': '1', 'NNGP_NM_LEVEL2': '0'},
    'spec2w2': {'NNGP_NM_SPEC': '1', 'NNGP_NM_LEVEL2': '2'},
    'spec2w4': {'NNGP_NM_SPEC': '1', 'NNGP_NM_LEVEL2': '4'},
    'fused': dict(_PACKED),
    'packed_queue': dict(_PACKED, NNGP_NM_REFILL='8'),
    'packed_static': dict(_PACKED, NNGP_NM_REFILL='0'),
    'park_w4': dict(_PARK, NNGP_RESUME_W4='100000', NNGP_RESUME_W2='100000'),
    'park_w2': dict(_PARK, NNGP_RESUME_W4='0', NNGP_RESUME_W2='100000'),
    'park_w1': dict(_PARK, NNGP_RESUME_W4='0', NNGP_RESUME_W2='0'),
    'lanes4': {'NNGP_NM_SPEC': '0', 'NNGP_NM_LANES': '1', 'NNGP_NM_LPF': '4'},
    'lanes1': {'NNGP_NM_SPEC': '0', 'NNGP_NM_LANES': '1', 'NNGP_NM_LPF': '1'},
}
# every knob the dispatch reads: a test clears the ones its form does not set
FORM_KNOBS = ('NNGP_NM_SPEC', 'NNGP_NM_LEVEL2', 'NNGP_NM_PARK', 'NNGP_NM_REFILL', 'NNGP_RESUME_W4',
              'NNGP_RESUME_W2', 'NNGP_NM_LANES', 'NNGP_NM_LPF')


def form_accepts(form, m):
    """Does the form exist for m (the two-level kernels: MAXM <= 32; the lanes kernels: m = 10, 15;
    park_w4 / park_w2 differ from park_w1 only where the two-level resume exists)?"""
    if form in ('spec2w2', 'spec2w4', 'park_w4', 'park_w2'):
        return m <= 32
    if form in ('lanes4', 'lanes1'):
        return m in LANE_MS
    return True


def refusing_shape(m):
    """(n_jitter, R) of the smallest prediction whose coordinate the fused kernel refuses (more
    fits than one workgroup may hold): the packed forms of nngp_predict."""
    M = maxm_for(m)
    return (9, 4) if M <= 16 else ((9, 2) if M <= 32 else (5, 1))


def fusing_shape(m):
    """(n_jitter, R) of the largest prediction the fused kernel still accepts."""
    M = maxm_for(m)
    return (9, 3) if M <= 16 else ((9, 1) if M <= 32 else (4, 1))


def form_shape(form, m):
    """(n_jitter, R) at which nngp_predict reaches `form` for m: nine jitters and one restart,
    except the packed forms, which need a coordinate the fused kernel refuses."""
    return refusing_shape(m) if form in ('packed_queue', 'packed_static') else (9, 1)


# ------------------------------------------------------------------------------ host dispatch
def _env(knobs, name, default):
    v = knobs.get(name)
    return default if v is None else int(v)


def _cus(ncu, what):
    if ncu is None:
        raise ValueError(f'{what} depends on the CU count under these knobs')
    return ncu


def _fused_launch(m, d, n_jitter, R, ncu):
    """run_nm(fused = true): (cpw, threads, nblocks), or None where it refuses."""
    M = maxm_for(m)
    nfc = n_jitter * R
    thr = lambda c: (c * nfc * 16 + 63) // 64 * 64
    lds = lambda t: 8 * (m * m + m + 4 * (t // 16) + (t // 16) * k_image_doubles(M))
    bad = lambda c: lds(thr(c)) > 150 * 1024 or thr(c) > nm_tmax(M)
    # one coordinate per workgroup while d <= #CU: every card has more than 3 CUs
    cpw = 1 if d <= 3 else max(1, min((d + _cus(ncu, 'cpw') - 1) // ncu, d))
    while cpw > 1 and bad(cpw):
        cpw -= 1
    if bad(cpw):
        return None
    return cpw, thr(cpw), (d + cpw - 1) // cpw


def _spec(m, n_fits, knobs, ncu, resume=False, nq=1):
    """run_nm_spec: the kernel that runs (or resumes) the fits, a wave or W waves per fit."""
    M = maxm_for(m)
    level2 = _env(knobs, 'NNGP_NM_LEVEL2', 1)
    if resume and nq == 1 and M <= 32 and level2 != 0:
        if 'NNGP_RESUME_W4' not in knobs or 'NNGP_RESUME_W2' not in knobs:
            _cus(ncu, 'resume_bounds')
        t4 = max(0, _env(knobs, 'NNGP_RESUME_W4', ncu))
        t2 = max(t4, _env(knobs, 'NNGP_RESUME_W2', 2 * (ncu or 0)))
        if t2 > 0:
            return ('nm_spec2_kernel', M, 0)
    if M > 32 or resume or level2 == 0:
        W = 1
    elif level2 in (2, 4):
        W = level2
    else:
        total = n_fits * nq
        _cus(ncu, 'spec_waves')
        W = 4 if total <= ncu else (2 if total <= (4 if M > 16 else 2) * ncu else 1)
    return ('nm_spec2_kernel', M, W) if W > 1 else ('nm_spec_kernel', M)


def _use_spec(m, n_fits, knobs, ncu):
    forced = _env(knobs, 'NNGP_NM_SPEC', -1)
    if forced >= 0:
        return forced != 0
    M = maxm_for(m)
    return n_fits <= (8 if M <= 16 else (4 if M <= 32 else 1)) * _cus(ncu, 'use_spec')


def _lanes(m, knobs):
    if _env(knobs, 'NNGP_NM_LPF', 4) == 1:
        return ('nm_lane1_kernel', m)
    return ('nm_lane_kernel', m, 4)


def _packed(m, n_fits, knobs, park_cap, nq=1):
    """run_nm(fused = false): (kernels, mode, threads, nblocks)."""
    M = maxm_for(m)
    if park_cap and nq == 1:
        return [('nm_fit_kernel', M, False)], 'park', 64, (n_fits + 3) // 4
    lanes = _env(knobs, 'NNGP_NM_LANES', -1)
    if lanes != 0 and m in LANE_MS and (lanes == 1 or n_fits * nq >= 16384):
        return [_lanes(m, knobs)], 'lanes', None, None
    threads = min(256, nm_tmax(M))
    nblocks = (n_fits + threads // 16 - 1) // (threads // 16)
    per_row = max(0, _env(knobs, 'NNGP_NM_REFILL', 8))
    if per_row > 1 and nblocks > 1:
        return [('nm_fit_kernel', M, False)], 'queue', threads, max(1, (nblocks + per_row - 1) // per_row)
    return [('nm_fit_kernel', M, False)], 'static', threads, nblocks


def _parked(m, n_fits, knobs, ncu):
    """run_nm_parked: the packed fits of one prediction, then the resume of the parked ones."""
    if _env(knobs, 'NNGP_NM_LANES', -1) == 1 and m in LANE_MS:
        return [_lanes(m, knobs)], 'lanes', None, None
    cap = max(0, _env(knobs, 'NNGP_NM_PARK', 70))
    if cap <= 0:
        return _packed(m, n_fits, knobs, 0)
    ker, mode, threads, nblocks = _packed(m, n_fits, knobs, cap)
    return ker + [_spec(m, n_fits, knobs, ncu, resume=True)], mode, threads, nblocks


def expected_form(m, d, n_jitter, R, knobs, api='predict', n_fits=None, ncu=None):
    """The host dispatch of nngp_predict (api = 'predict': d * n_jitter * R fits) or of
    nngp_nm_fit_batch (api = 'fit_batch': n_fits fits) under the environment `knobs`, restated:
    dict(rc, kernels = [(template, MAXM or m, parameter ...) in launch order], mode, threads,
    nblocks, cpw).  ncu = None: raise where a branch would depend on the CU count."""
    assert 1 <= m <= MAX_M and 1 <= n_jitter <= MAX_JIT and R >= 1
    M = maxm_for(m)
    out = dict(rc=NNGP_OK, mode=None, threads=None, nblocks=None, cpw=None)
    if api == 'fit_batch':
        if _use_spec(m, n_fits, knobs, ncu):
            out.update(kernels=[_spec(m, n_fits, knobs, ncu)], mode='spec')
        else:
            ker, mode, threads, nblocks = _parked(m, n_fits, knobs, ncu)
            out.update(kernels=ker, mode=mode, threads=threads, nblocks=nblocks)
        return out
    n_fits = d * n_jitter * R
    mean = ('gp_mean_kernel', M)
    if _use_spec(m, n_fits, knobs, ncu):
        out.update(kernels=[_spec(m, n_fits, knobs, ncu), mean], mode='spec')
        return out
    if max(0, _env(knobs, 'NNGP_NM_PARK', 70)) == 0:
        fl = _fused_launch(m, d, n_jitter, R, ncu)
        if fl is not None:
            out.update(kernels=[('nm_fit_kernel', M, True)], mode='fused', cpw=fl[0], threads=fl[1], nblocks=fl[2])
            return out
    ker, mode, threads, nblocks = _parked(m, n_fits, knobs, ncu)
    out.update(kernels=ker + [mean], mode=mode, threads=threads, nblocks=nblocks)
    return out


def sweep_kernels(m, knobs):
    """Fit-side kernels a direct nngp_correction_sweep with speculation on launches at m whatever
    the hit pattern: the packed batch of every guessed query's fits (nq > 1: no parking) and,
    by the knobs, the query-independent half of the hit slices' means or the fused chain."""
    M = maxm_for(m)
    chained = _env(knobs, 'NNGP_CHAIN', 0) != 0 and m <= CHAIN_MAX_M
    out = [('nm_fit_kernel', M, False)]
    if chained:
        out.append(('chain_kernel', M))
    elif _env(knobs, 'NNGP_RESPEC_W', 4) > 0 and _env(knobs, 'NNGP_HIT_MEAN', 1) != 0:
        out.append(('gp_pre_kernel', M))
    return out


# ------------------------------------------------------------------------------- the matrices
FUSED_D257_MS = (8, 16)   # cpw = 2 on a 256-CU card, the last workgroup with one coordinate
FUSED_D257_CUS = 256


def predict_rows():
    """The rows of the nngp_predict matrix: (m, variant, form, d, n_jitter, R)."""
    rows = []
    for m in ALL_MS:
        for variant in ('smooth', 'dup'):
            for form in ('spec1', 'fused', 'park_w4'):
                rows.append((m, variant, form, 3, 9, 1))
    for m in EDGE_MS:
        for variant in ('smooth', 'dup'):
            for form in ('spec2w2', 'spec2w4', 'park_w2', 'park_w1', 'packed_queue', 'packed_static'):
                if form_accepts(form, m):
                    rows.append((m, variant, form, 3) + form_shape(form, m))
            # the fused kernel's edge: the largest coordinate it accepts, the smallest it refuses
            for nj, R in (fusing_shape(m), refusing_shape(m)):
                if (nj, R) != (9, 1):
                    rows.append((m, variant, 'fused', 3, nj, R))
    for m in LANE_MS:
        for variant in ('smooth', 'dup'):
            for form in ('lanes4', 'lanes1'):
                rows.append((m, variant, form, 3, 9, 1))
    for m in FUSED_D257_MS:
        rows.append((m, 'smooth', 'fused', 257, 9, 1))
    return rows


def predict_row_id(row):
    m, variant, form, d, nj, R = row
    return f'm{m}-{variant}-{form}' + (f'-d{d}' if d != 3 else '') + (f'-j{nj}R{R}' if (nj, R) != (9, 1) else '')


# caps and tolerances: (fatol = xatol, maxfev).  maxfev 9, 10, 11 lie below, at and above the park
# point of the park forms (NNGP_NM_PARK = 10); tolerance 0 ends a fit by the iteration rule alone,
# tolerance 1e9 at the first check
CAP_SETTINGS = ([(0.1, k) for k in (1, 2, 3, 4, 5, 9, 10, 11)] + [(0.0, 60), (1e9, 400)])
CAP_FORMS = ('spec1', 'spec2w2', 'spec2w4', 'fused', 'packed_queue', 'packed_static', 'park_w4', 'park_w2',
             'park_w1', 'lanes4', 'lanes1')


def cap_rows():
    """(m, variant, form) of the caps-and-tolerances matrix: every form at the edge m it accepts
    (the lanes kernels at their two m)."""
    return [(m, variant, form) for m in sorted(set(EDGE_MS) | set(LANE_MS)) for form in CAP_FORMS
            for variant in ('dup', 'zero')
            if form_accepts(form, m) and (m in EDGE_MS or form in ('lanes4', 'lanes1'))]


BATCH_MS = (1, 8, 9, 16, 20, 32, 33, 64)
BATCH_D = 5
BATCH_NFITS = (1, 3, 4, 5, 16, 17, 33, 64, 65)
BATCH_NJ = (1, 9, MAX_JIT)
BATCH_FORMS = ('spec1', 'spec2w4', 'park_w4', 'packed_queue', 'packed_static')


def batch_rows():
    """(m, form) of the nngp_nm_fit_batch matrix."""
    rows = [(m, form) for m in BATCH_MS for form in BATCH_FORMS if form_accepts(form, m)]
    return rows + [(m, form) for m in LANE_MS for form in ('lanes4', 'lanes1')]


# ---------------------------------------------------------------------- the 'scale' family
# Fits and means whose Cholesky pivots leave the range of the short sqrt / reciprocal sequences
# (csrc/nngp_math.h in_mid_range: 2^-500 <= x < 2^500 (1 + 2^-20), i.e. 3.05e-151 .. 3.27e150), so
# nngp_gpeval.h's wave-wide ballot falls back to sqrt() and 1.0 / ljj and the lanes kernels'
# sqrt_rcp_exact rescales by 4^+-300.  Three kinds of fit, interleaved so that adjacent fits always
# differ in kind -- a wave of four fits then holds in-range and out-of-range pivots at once:
#   'ord'   sy in -8 .. -1, jitter 1e-20 or 1e-12 (every pivot in range)
#   'high'  sy in SCALE_HIGH_SY: psy = 10^sy > 2^500 (1 + 2^-20).  10^150.6 = 3.98e150 is so close
#           above it that the pivots of later columns (a_jj minus the squares of the row) are back
#           inside: such a matrix crosses the boundary in the middle of its factorisation
#   'low'   sy in SCALE_LOW_SY with the 1e-170 jitter: psy + jitter < 2^-500
# on the 'smooth' set (well-conditioned at sx = -3, -2, so every -LML is finite).
SCALE_JITTERS = np.array([-170.0, -20.0, -12.0])
SCALE_HIGH_SY = (150.6, 151.0, 160.0)
SCALE_LOW_SY = (-151.0, -160.0)
SCALE_SX = (-3.0, -2.0)
SCALE_MS = (10, 15, 20, 33, 64)           # (33, 64: the nn_exp_nonpos_sep kernels; 10, 15: the lanes kernels)
SCALE_NFITS = 19                          # five waves of four, the last partial; two workgroups up to M = 32
SCALE_SETTINGS = tuple((0.1, k) for k in (3, 9, 11, 400))
SCALE_KINDS = ('ord', 'high', 'low')
MID_LO, MID_HI = float.fromhex('0x1p-500'), float.fromhex('0x1.00001p+500')


def mid_accepts(x):
    """csrc/nngp_math.h in_mid_range, restated."""
    return MID_LO <= x < MID_HI


def scale_thetas(n, seed):
    """(kind [n], jitter_idx [n], theta [n][2]): fit i is of kind SCALE_KINDS[i % 3]."""
    rng = np.random.default_rng(seed)
    kind = [SCALE_KINDS[i % 3] for i in range(n)]
    jidx = np.zeros(n, dtype=np.int32)
    theta = np.zeros((n, 2))
    for i, k in enumerate(kind):
        theta[i, 0] = SCALE_SX[int(rng.integers(0, 2))]
        if k == 'ord':
            theta[i, 1], jidx[i] = float(rng.integers(-8, 0)), 1 + (i // 3) % 2
        elif k == 'high':
            theta[i, 1], jidx[i] = SCALE_HIGH_SY[(i // 3) % 3], (i // 3 + 1) % 3
        else:
            theta[i, 1], jidx[i] = SCALE_LOW_SY[(i // 3) % 2], 0
    return kind, jidx, theta


def scale_pivots(D2, theta, jitter_exp):
    """The Cholesky pivots of K = psy exp(c D2) + jitter I by the oracle (orc_potf2 on the matrix
    gp_factor builds): pivot 0 exactly, the later ones as L_jj^2; None where the factorisation fails."""
    import ctypes
    import oracle as O
    L = O.lib()
    m = D2.shape[0]
    c = -0.5 * (1 / L.nn_pow10(float(theta[0])))
    psy = L.nn_pow10(float(theta[1]))
    K = np.array([[psy * L.nn_exp(c * D2[r, j]) for j in range(m)] for r in range(m)])
    K[np.diag_indices(m)] += float(10.0 ** jitter_exp)
    first = float(K[0, 0])
    rinv = np.empty(m)
    dp = ctypes.POINTER(ctypes.c_double)
    if L.orc_potf2(m, K.ctypes.data_as(dp), rinv.ctypes.data_as(dp)):
        return None
    d = np.diag(K)
    return np.concatenate([[first], d[1:] * d[1:]])


def _check_scale_conditions(D2, kind, jidx, theta, need_crossing):
    """Conditions on the recipe, from the oracle: every high or low matrix starts outside the set
    in_mid_range accepts and, for the fit lists, some sy = 150.6 matrix comes back inside it at a
    later column."""
    crossing = 0
    for k, a, th in zip(kind, jidx, theta):
        piv = scale_pivots(D2, th, SCALE_JITTERS[a])
        assert piv is not None, (k, th)
        inside = [mid_accepts(p) for p in piv]
        if k == 'ord':
            assert all(inside), (k, th)
            continue
        assert not inside[0], (k, th, piv[0])
        assert (piv[0] > MID_HI) == (k == 'high')
        # (a margin of 1e-9 relative: L_jj^2 is the pivot up to two roundings)
        if th[1] == 150.6 and any(mid_accepts(p * (1 - 1e-9)) and mid_accepts(p * (1 + 1e-9)) for p in piv[1:]):
            crossing += 1
    assert crossing >= 1 or not need_crossing


@functools.lru_cache(maxsize=None)
def scale_fit_case(m):
    """(xm, ym, coord, jitter_idx, theta0, kind) of the SCALE_NFITS fits at m neighbours."""
    import oracle as O
    xm, ym, _ = fit_case(m, BATCH_D, 'smooth')
    kind, jidx, theta0 = scale_thetas(SCALE_NFITS, 7000 + m)
    coord = np.random.default_rng(7100 + m).integers(0, BATCH_D, SCALE_NFITS).astype(np.int32)
    assert all(kind[i] != kind[i + 1] for i in range(SCALE_NFITS - 1))
    D2 = O.d2_matrix(xm)
    _check_scale_conditions(D2, kind, jidx, theta0, True)
    for f in range(SCALE_NFITS):
        assert np.isfinite(O.nlml(D2, ym[:, coord[f]], theta0[f], SCALE_JITTERS[jidx[f]])), (m, f)
    for a in (xm, ym, coord, jidx, theta0):
        a.setflags(write=False)
    return xm, ym, coord, jidx, theta0, tuple(kind)


@functools.lru_cache(maxsize=None)
def scale_fit_oracle(m, fatol, maxfev):
    """(theta [n][2], -LML [n], nfev [n]) of the oracle's Nelder-Mead on scale_fit_case(m): every
    form shares this expectation.  Every fit ends at a finite -LML."""
    import oracle as O
    xm, ym, coord, jidx, theta0, _ = scale_fit_case(m)
    D2 = O.d2_matrix(xm)
    res = [O.nm_fit(D2, ym[:, coord[f]], theta0[f], SCALE_JITTERS[jidx[f]], fatol, fatol, maxfev)
           for f in range(SCALE_NFITS)]
    out = (np.array([r[0] for r in res]).reshape(-1, 2), np.array([r[1] for r in res]),
           np.array([r[2] for r in res], dtype=np.int32))
    assert np.isfinite(out[1]).all(), (m, maxfev)
    for a in out:
        a.setflags(write=False)
    return out


def scale_rows():
    """(m, form) of the 'scale' matrix: every form that exists for m."""
    return [(m, form) for m in SCALE_MS for form in FORMS if form_accepts(form, m)]


SCALE_MEAN_D = 13     # more than three waves of four coordinates, the last one partial


@functools.lru_cache(maxsize=None)
def scale_mean_case(m):
    """(xm, ym, q, theta [d][2], jitter_idx [d], the oracle's means [d], kind) for nngp_gp_mean with
    the same interleaved thetas; one case per padded size (m = the size itself)."""
    import oracle as O
    d = SCALE_MEAN_D
    xm, ym, q = fit_case(m, d, 'smooth')
    kind, jidx, theta = scale_thetas(d, 7200 + m)
    _check_scale_conditions(O.d2_matrix(xm), kind, jidx, theta, False)
    want = np.array([O.gp_mean(xm, ym[:, c], q, theta[c], SCALE_JITTERS[jidx[c]]) for c in range(d)])
    assert np.isfinite(want).all(), m
    return xm, ym, q, theta, jidx, want, tuple(kind)


MEAN_D = (1, 3, 4, 5, 15, 16, 17, 33)
# with the smallest jitter the coinciding pair of 'dup' fails the Cholesky at every m >= 3 under the
# first; under the others it fails at most m and passes on rounding noise at the rest
SINGULAR_THETA = (6.0, 2.0)
NEAR_SINGULAR_THETAS = ((2.0, -1.0), (0.0, 0.0), (-2.0, -1.0))
SWEEP_MS = (8, 16, 20, 24, 32, 33, 64)


def instantiations():
    """Every (kernel template, MAXM or m, parameter ...) the tables above reach, by expected_form
    and sweep_kernels."""
    seen = set()
    for m, _, form, d, nj, R in predict_rows():
        ncu = FUSED_D257_CUS if d > 3 else None
        seen.update(expected_form(m, d, nj, R, FORMS[form], ncu=ncu)['kernels'])
    for m, form in batch_rows():
        for n in BATCH_NFITS:
            seen.update(expected_form(m, BATCH_D, 9, 1, FORMS[form], api='fit_batch', n_fits=n)['kernels'])
    for m, form in scale_rows():
        seen.update(expected_form(m, BATCH_D, len(SCALE_JITTERS), 1, FORMS[form], api='fit_batch',
                                  n_fits=SCALE_NFITS)['kernels'])
    for m in SWEEP_MS + (18,):   # (m = 18: the sweeps of tests/test_gpu_knn_matrix.py)
        for knobs in ({}, {'NNGP_HIT_MEAN': '0'}, {'NNGP_CHAIN': '1'}):
            seen.update(sweep_kernels(m, knobs))
    return seen


# --------------------------------------------------------------------------- oracle results
@functools.lru_cache(maxsize=None)
def oracle_predict(m, variant, d, n_jitter, R, fatol, xatol, maxfev):
    """(preds, fits) of the oracle for a prediction case: every form shares this expectation."""
    import oracle as O
    X, Y, q, th0 = predict_case(m, variant, d, n_jitter, R)
    preds, fits = O.predict(X, Y, q, m, th0, n_restarts=R, fatol=fatol, xatol=xatol, maxfev=maxfev,
                            return_fits=True, jitters=jitters_for(n_jitter))
    preds.setflags(write=False)
    fits.setflags(write=False)
    return preds, fits
