"""Inputs of tests/test_gpu_math_probe.py: for every routine of csrc/nngp_math.h the random sets
(fixed seeds, at most 2^22 points per routine) and the curated ones -- thresholds, clamps, rint
ties of the reductions, quadrant edges, binade ends, rounding ties of sqrt and the reciprocal,
subnormals, zeros of both signs, infinities and NaNs.  No GPU is needed to build a set; every
builder returns float64 arrays that the caller must not change (they are cached)."""
import functools

import numpy as np

N_RANDOM = 1 << 22

# csrc/nngp_math.h MathC, restated
LN2 = float(np.log(2.0))
LN10 = float.fromhex('0x1.26bb1bbb55516p+1')
LN10_LO = float.fromhex('-0x1.f48ad494ea3e9p-53')
EXP_OVF = 709.782712893384
EXP_UNF = -745.1332191019412
EXP_CLAMP_LO, EXP_CLAMP_HI = -746.0, 710.0
LN_DBL_MIN = -1022 * LN2                      # ln(2^-1022): below it the result is subnormal

DBL_MAX = float(np.finfo(float).max)
DBL_MIN = float(np.finfo(float).tiny)
DENORM_MIN = float.fromhex('0x1p-1074')
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan])

# the set in_mid_range accepts: one unsigned compare on the high word, so 2^500's whole first
# 2^-20 of a binade passes
MID_LO = float.fromhex('0x1p-500')
MID_HI = float.fromhex('0x1.00001p+500')      # 2^500 (1 + 2^-20): the first double refused
MID_ES = (-500, -499, -251, -250, -1, 0, 1, 250, 251, 499, 500)


def mid_accepts(x):
    """The predicate csrc/nngp_math.h in_mid_range implements (NaN: False)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return (x >= MID_LO) & (x < MID_HI)


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    a.setflags(write=False)
    return a


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint64).view(np.float64)


def around(x, k):
    """Every x and its k neighbours on either side (np.nextafter, so zeros, the subnormal range and
    the infinities are crossed as the number line has them)."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo = np.nextafter(lo, -np.inf)
        hi = np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


def two_prod_err(a, b):
    """fma(a, b, -(a*b)) for arrays, by Dekker's splitting: exact while nothing over- or underflows
    (|a|, |b| and |a*b| between 2^-900 and 2^900 here), and fma's NaN / inf otherwise."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all='ignore'):
        p = a * b
        ca, cb = 134217729.0 * a, 134217729.0 * b
        ah = ca - (ca - a)
        bh = cb - (cb - b)
        al, bl = a - ah, b - bh
        e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
        return np.where(np.isfinite(p) & (p != 0), e, p - p)


def random_patterns(rng, lo, hi, n):
    """n doubles whose bit patterns are uniform in [bits(lo), bits(hi)] (0 <= lo <= hi): uniform
    inside a binade and over the binades, i.e. log-uniform up to a factor of two."""
    b0, b1 = int(bits(lo)[0]), int(bits(hi)[0])
    return from_bits(rng.integers(b0, b1, n, dtype=np.uint64, endpoint=True))


# ----------------------------------------------------------------------------------------- exp
@functools.lru_cache(maxsize=None)
def exp_cases():
    rng = np.random.default_rng(101)
    k = np.arange(-1076, 1026, dtype=np.float64)
    sets = [
        rng.uniform(EXP_CLAMP_LO, EXP_CLAMP_HI, N_RANDOM // 2),
        rng.uniform(-1.0, 1.0, N_RANDOM // 2),
        np.linspace(-745.14, -708.39, 1 << 18),           # subnormal results
        around([EXP_OVF, EXP_UNF], 1),
        around([EXP_CLAMP_HI, EXP_CLAMP_LO, LN_DBL_MIN], 4),
        around(k * LN2, 1), around((k + 0.5) * LN2, 1),   # rint ties of the reduction, the sign of r
        [DENORM_MIN, -DENORM_MIN, 1e-300, -1e-300, 2.0 ** -54, -2.0 ** -54],
        SPECIALS,
    ]
    return _frozen(np.concatenate([np.asarray(s, dtype=np.float64) for s in sets]))


@functools.lru_cache(maxsize=None)
def exp_nonpos_cases():
    """exp_cases restricted to what NONPOS admits: x <= 0 (both zeros, -inf) and NaN."""
    x = exp_cases()
    with np.errstate(invalid='ignore'):
        keep = (x <= 0.0) | np.isnan(x)
    x = x[keep]
    assert np.any(bits(x) == bits(-0.0)[0]) and np.any(x == -np.inf) and np.any(np.isnan(x))
    return _frozen(x)


# --------------------------------------------------------------------------------------- 10^x
POW10_SCALE_EXPS = (160.0, -160.0, 170.0, -170.0)   # tests/nm_cases.py: the 'scale' family


@functools.lru_cache(maxsize=None)
def pow10_cases():
    rng = np.random.default_rng(102)
    sets = [
        rng.uniform(-330.0, 310.0, N_RANDOM),              # under- and overflows
        np.arange(-660, 621) / 2.0,                        # every integer and half-integer
        np.arange(-20.0, -10.0),                           # the jitter exponents
        np.arange(-10 * 1024, 2 * 1024 + 1) / 1024.0,      # the fit range, steps of 2^-10
        POW10_SCALE_EXPS, [150.6, 151.0, -151.0],
        SPECIALS,
    ]
    return _frozen(np.concatenate([np.asarray(s, dtype=np.float64) for s in sets]))


@functools.lru_cache(maxsize=None)
def exp_dd_cases():
    """(hi, lo): the pairs nn_pow10 forms (hi = x ln10, lo = fma(x, ln10, -hi) + x LN10_LO) from its
    own cases, and hi at the thresholds with lo = +-ulp(hi)/2."""
    x = pow10_cases()
    with np.errstate(all='ignore'):
        hi = x * LN10
        lo = two_prod_err(x, LN10) + x * LN10_LO
    th = around([EXP_OVF, EXP_UNF, EXP_CLAMP_HI, EXP_CLAMP_LO, LN_DBL_MIN, 0.0], 2)
    half = np.spacing(np.abs(th)) / 2
    hi = np.concatenate([hi, th, th, th])
    lo = np.concatenate([lo, half, -half, np.zeros_like(th)])
    return _frozen(hi), _frozen(lo)


# ----------------------------------------------------------------------------------------- log
@functools.lru_cache(maxsize=None)
def log_cases():
    rng = np.random.default_rng(103)
    rt = float(np.sqrt(0.5))                               # RN(sqrt(1/2)): the split of frexp's m
    sets = [
        np.exp(rng.uniform(-745.0, 709.0, N_RANDOM)),
        around(np.ldexp(1.0, np.arange(-1074, 1024)), 1),
        around(np.ldexp(rt, np.array([-1022, -1, 0, 1, 1023])), 2),
        from_bits(rng.integers(1, 1 << 52, 1 << 10, dtype=np.uint64)),   # subnormals
        around([1.0], 1), [DBL_MIN, DBL_MAX, -1.0],
        SPECIALS,
    ]
    return _frozen(np.concatenate([np.asarray(s, dtype=np.float64) for s in sets]))


# ---------------------------------------------------------------------------------- sin / cos
@functools.lru_cache(maxsize=None)
def trig_cases():
    rng = np.random.default_rng(104)
    k = np.arange(-4096, 4097, dtype=np.float64)
    p2 = np.ldexp(1.0, np.arange(0, 1024))
    big = np.array([1e22, 1e300, DBL_MAX])
    sets = [
        rng.uniform(-40.0, 40.0, N_RANDOM // 2),
        rng.uniform(-1e5, 1e5, N_RANDOM // 4),
        rng.uniform(-1e9, 1e9, N_RANDOM // 4),
        around(k * (np.pi / 4), 2),                        # quadrant edges, zero crossings
        p2, -p2, big, -big,                                # n + 1.5 2^52 for |n| >= 2^51 too
        from_bits(rng.integers(1, 1 << 52, 256, dtype=np.uint64)),
        -from_bits(rng.integers(1, 1 << 52, 256, dtype=np.uint64)),
        [DENORM_MIN, -DENORM_MIN, DBL_MIN, -DBL_MIN],
        SPECIALS,
    ]
    return _frozen(np.concatenate([np.asarray(s, dtype=np.float64) for s in sets]))


# ------------------------------------------------------------------------------- in_mid_range
@functools.lru_cache(maxsize=None)
def mid_range_cases():
    rng = np.random.default_rng(105)
    edges = around([MID_LO, float.fromhex('0x1.00001p-500'), float.fromhex('0x1p+500'), MID_HI], 2)
    nans = from_bits(np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001,
                               0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))
    sub = from_bits(rng.integers(1, 1 << 52, 64, dtype=np.uint64))
    other = np.array([1.0, DBL_MIN, DBL_MAX, DENORM_MIN, 1e-151, 1e-150, 1e150, 1e151])
    pos = np.concatenate([edges, sub, other, np.ldexp(1.0, np.arange(-1074, 1024))])
    anybits = from_bits(rng.integers(0, 1 << 64, 1 << 20, dtype=np.uint64))
    return _frozen(np.concatenate([pos, -pos, SPECIALS, nans, anybits]))


# ------------------------------------------------------------------------- sqrt_mid / rcp_mid
def _binade_ends():
    j = np.arange(0, 65, dtype=np.float64)
    return np.concatenate([np.ldexp(np.concatenate([1.0 + j * 2.0 ** -52, 2.0 - j * 2.0 ** -52]), e) for e in MID_ES])


def _accepted(sets):
    x = np.concatenate([np.asarray(s, dtype=np.float64) for s in sets])
    return x[mid_accepts(x)]


@functools.lru_cache(maxsize=None)
def _mid_common():
    """The sets sqrt_mid and rcp_mid share, before the filter to what in_mid_range accepts."""
    rng = np.random.default_rng(106)
    k = np.concatenate([np.arange(1.0, 4097.0), rng.integers(1, 1 << 26, 1 << 12).astype(np.float64)])
    return [
        random_patterns(rng, MID_LO, np.nextafter(MID_HI, 0.0), N_RANDOM),
        _binade_ends(),
        around(k * k, 1),                                  # perfect squares (exact: k < 2^26.5)
        around([MID_LO, float.fromhex('0x1p+500')], 2), [np.nextafter(MID_HI, 0.0)],
    ]


@functools.lru_cache(maxsize=None)
def _near_square_ys():
    rng = np.random.default_rng(107)
    return random_patterns(rng, float.fromhex('0x1p-250'), float.fromhex('0x1p+250'), 1 << 16)


@functools.lru_cache(maxsize=None)
def sqrt_mid_cases():
    y = _near_square_ys()
    return _frozen(_accepted(_mid_common() + [around(y * y, 1)]))    # RN(y^2): near rounding ties


@functools.lru_cache(maxsize=None)
def rcp_mid_cases():
    rng = np.random.default_rng(108)
    y = random_patterns(rng, MID_LO, np.nextafter(MID_HI, 0.0), 1 << 16)
    # what gpeval feeds it: the square roots of sqrt_mid's curated arguments, in [2^-250, 2^250]
    curated = np.concatenate([np.asarray(s, dtype=np.float64) for s in _mid_common()[1:]])
    ys = _near_square_ys()
    fed = np.sqrt(np.concatenate([curated[mid_accepts(curated)], around(ys * ys, 1), _mid_common()[0][:1 << 16]]))
    return _frozen(_accepted(_mid_common() + [around(1.0 / y, 1), fed]))


# ---------------------------------------------------------------------------- sqrt_rcp_exact
@functools.lru_cache(maxsize=None)
def sqrt_rcp_cases():
    """Every x > 0: the subnormals, the k = +300 / 0 / -300 switch at 2^-500 and 2^500, DBL_MAX, +inf."""
    rng = np.random.default_rng(109)
    sets = [
        random_patterns(rng, DENORM_MIN, DBL_MAX, N_RANDOM),
        from_bits(rng.integers(1, 1 << 52, 1 << 10, dtype=np.uint64)),
        [DENORM_MIN, np.nextafter(DBL_MIN, 0.0), DBL_MIN, np.nextafter(DBL_MIN, 1.0)],
        around([MID_LO, float.fromhex('0x1p+500'), MID_HI], 2),
        np.ldexp(1.0, np.arange(-1074, 1024)), _binade_ends(),
        [np.nextafter(DBL_MAX, 0.0), DBL_MAX, np.inf],
    ]
    x = np.concatenate([np.asarray(s, dtype=np.float64) for s in sets])
    assert np.all(x > 0)
    return _frozen(x)
