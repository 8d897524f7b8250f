"""CPU checks behind tests/test_gpu_math_probe.py: the sets of tests/math_cases.py hold the points
the GPU tests are about, the oracle's array entry points are its scalar routines, and the pairs
built for nn_exp_dd are the ones nn_pow10 forms."""
import ctypes

import numpy as np

import math_cases as MC
import oracle as O

_dp = ctypes.POINTER(ctypes.c_double)


def _arr(fn, *args, n_out=1):
    args = [np.ascontiguousarray(a, dtype=np.float64) for a in args]
    outs = [np.full(args[0].shape, -7.0) for _ in range(n_out)]
    getattr(O.lib(), fn)(args[0].size, *[a.ctypes.data_as(_dp) for a in args], *[o.ctypes.data_as(_dp) for o in outs])
    return outs[0] if n_out == 1 else outs


def _has(x, v):
    return bool(np.any(MC.bits(x) == MC.bits(np.array([v]))[0]))


def _same(a, b):
    return bool(np.all((MC.bits(a) == MC.bits(b)) | (np.isnan(a) & np.isnan(b))))


def test_sets_hold_their_edges():
    x = MC.exp_cases()
    for v in (MC.EXP_OVF, np.nextafter(MC.EXP_OVF, np.inf), MC.EXP_UNF, np.nextafter(MC.EXP_UNF, -np.inf), 710.0, -746.0,
              0.0, -0.0, np.inf, -np.inf, MC.DENORM_MIN, -1076 * MC.LN2, 1025.5 * MC.LN2):
        assert _has(x, v), v
    assert np.isnan(x).any() and x.size <= MC.N_RANDOM + (1 << 19)
    e = _arr('orc_exp_array', x)
    assert ((e > 0) & (e < MC.DBL_MIN)).sum() > 1 << 18          # subnormal results, densely
    n = MC.exp_nonpos_cases()
    assert np.all((n <= 0) | np.isnan(n)) and _has(n, -0.0) and _has(n, -np.inf) and _has(n, MC.EXP_UNF)
    p = MC.pow10_cases()
    for v in (-330.0, 310.0, 0.5, -20.0, -11.0, 160.0, -170.0, 150.6, -10.0 + 2.0 ** -10, 0.0, -0.0, np.inf, -np.inf):
        assert _has(p, v), v
    lg = MC.log_cases()
    for v in (MC.DENORM_MIN, MC.DBL_MIN, MC.DBL_MAX, 1.0, np.nextafter(1.0, 0), np.nextafter(1.0, 2), np.sqrt(0.5),
              np.nextafter(np.sqrt(0.5), 0), np.sqrt(0.5) * 2.0 ** 1023, 0.0, -0.0, -1.0, np.inf, -np.inf):
        assert _has(lg, v), v
    assert ((lg > 0) & (lg < MC.DBL_MIN)).sum() >= 1 << 10
    t = MC.trig_cases()
    for v in (np.pi / 4, np.nextafter(np.pi, 4), -4096 * (np.pi / 4), 2.0 ** 51, -2.0 ** 1023, 1e22, -1e300, MC.DBL_MAX,
              MC.DENORM_MIN, 0.0, -0.0, np.inf, -np.inf):
        assert _has(t, v), v
    assert (np.abs(t) > 1e5).sum() >= 1 << 19 and (np.abs(t) <= 40).sum() >= 1 << 21


def test_mid_range_sets():
    lo, hi = 2.0 ** -500, 2.0 ** 500
    assert MC.MID_LO == lo and MC.MID_HI == hi * (1 + 2.0 ** -20)
    # the predicate is the compare on the high word: 0x20B00000 <= high word <= 0x5F300000
    x = MC.mid_range_cases()
    hw = (MC.bits(x) >> np.uint64(32)).astype(np.int64)
    assert np.array_equal(MC.mid_accepts(x), (hw >= 0x20B00000) & (hw <= 0x5F300000))
    for v in (lo, np.nextafter(lo, 0), hi, np.nextafter(MC.MID_HI, 0), MC.MID_HI, -lo, -hi, 0.0, -0.0, np.inf, -np.inf):
        assert _has(x, v), v
    assert np.isnan(x).sum() >= 7 and np.signbit(x[np.isnan(x)]).any() and not np.signbit(x[np.isnan(x)]).all()
    for s in (MC.sqrt_mid_cases(), MC.rcp_mid_cases()):
        assert MC.mid_accepts(s).all() and _has(s, lo) and _has(s, np.nextafter(MC.MID_HI, 0)) and _has(s, hi)
        assert _has(s, 2.0 - 2.0 ** -52) and _has(s, (1 + 2.0 ** -52) * 2.0 ** -251) and _has(s, 49.0)
    r = MC.rcp_mid_cases()
    assert ((r >= 2.0 ** -250) & (r <= 2.0 ** 250)).sum() > 1 << 21
    q = MC.sqrt_rcp_cases()
    assert q[-1] == np.inf and np.all(q > 0) and _has(q, MC.DENORM_MIN) and _has(q, MC.DBL_MAX)
    assert (q < lo).sum() > 1 << 20 and (q > hi).sum() > 1 << 20 and _has(q, np.nextafter(lo, 0)) and _has(q, np.nextafter(hi, np.inf))


def test_oracle_array_entry_points_are_the_scalar_routines():
    L = O.lib()
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-320, 320, 2000), MC.SPECIALS, [150.6, -170.0]])
    assert _same(_arr('orc_pow10_array', x), np.array([L.nn_pow10(float(v)) for v in x]))
    assert _same(_arr('orc_exp_dd_array', x, np.zeros_like(x)), np.array([L.nn_exp(float(v)) for v in x]))
    t = np.concatenate([rng.uniform(-1e5, 1e5, 2000), MC.SPECIALS, [1e22, 2.0 ** 1000]])
    sn, cs = _arr('orc_sincos_array', t, n_out=2)
    assert _same(sn, np.array([L.nn_sin(float(v)) for v in t])) and _same(cs, np.array([L.nn_cos(float(v)) for v in t]))
    assert _same(_arr('orc_sin_pi_array', t), np.array([L.nn_sin_pi(float(v)) for v in t]))


def test_exp_dd_pairs_are_the_ones_pow10_forms():
    """nn_exp_dd on the (hi, lo) built with Dekker's product is nn_pow10 on the x they came from."""
    x = MC.pow10_cases()
    hi, lo = MC.exp_dd_cases()
    assert _same(_arr('orc_exp_dd_array', hi[:x.size], lo[:x.size]), _arr('orc_pow10_array', x))
    th = hi[x.size:]
    assert _has(th, MC.EXP_OVF) and _has(th, MC.EXP_UNF) and np.all(np.abs(lo[x.size:]) <= np.spacing(np.abs(th)) / 2)
    assert (lo[x.size:] > 0).any() and (lo[x.size:] < 0).any()
