"""The arithmetic of the Hopf group kernel's time track (csrc/nngp_rk_kernels.h, GroupSys<HOPF>:
track_div, f_take; rk_group_kernel: TRACK), restated in numpy on the host and checked against the
CPU oracle.

Hopf's third component has f = 1, so in fixed-step mode RK4 adds the same INC = RN(sum b k) to u2 at
every step, whatever u0 and u1 do.  The kernel therefore keeps the time inputs of four steps in 16
lanes of one register (lane 4j + r: step j; r = 0 stage 0, r = 1 stages 1 and 2, r = 2 stage 3),
de-normalises and divides them by mu once, and advances the register by sequential adds of INC.
Here the same expressions run on numpy doubles, 16 lanes as a vector; the fused multiply-adds of
the Markstein division are formed exactly (fractions) and rounded once."""
from fractions import Fraction

import numpy as np

import oracle as O

MU = 500.0
R = 1.0 / MU                                    # rparam0
MN, MX = (np.asarray(b, dtype=float) for b in O.BOUNDS['hopf'][:2])
MN2, HW2, SC2 = MN[2], 0.5 * (MX[2] - MN[2]), 2 / (MX[2] - MN[2])   # the kernel's mn, hw, sc of component 2
NEG0 = -0.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _fma(a, b, c):
    """RN(a*b + c) for finite doubles, the sign of an exact zero by the IEEE rule"""
    a, b, c = float(a), float(b), float(c)
    s = Fraction(a) * Fraction(b) + Fraction(c)
    if s != 0:
        return float(s)
    pneg = bool(np.signbit(a)) != bool(np.signbit(b))
    if a * b == 0 and c == 0:
        return NEG0 if (pneg and bool(np.signbit(c))) else 0.0
    return 0.0


def _div_mu(x):
    """div_const(x, mu, RN(1/mu)), per lane"""
    out = np.empty_like(x)
    for i, v in enumerate(x):
        q = np.float64(v) * R
        out[i] = _fma(_fma(-q, MU, v), R, q)
    return out


def _constants(dt, norm):
    """INC and the two stage offsets from the step's own expressions (folded tableau)"""
    dt = np.float64(dt)
    o = np.float64(1.0) * SC2 if norm else np.float64(1.0)
    k0 = (0.5 * dt) * o
    k1 = (0.5 * dt) * o
    k2 = dt * o
    k3 = dt * o
    inc = (((1.0 / 3) * k0 + (2.0 / 3) * k1) + (1.0 / 3) * k2) + (1.0 / 6) * k3
    kc = dt * o
    return inc, 0.5 * kc, 1.0 * kc


def _denorm(x, norm):
    return (x + 1) * HW2 + MN2 if norm else x


def _track_spread(u2, inc):
    """the track at the start of a pass: lane 4j + r holds u2 after j steps"""
    j = np.arange(16) >> 2
    tu = np.full(16, u2, dtype=np.float64)       # row_newbcast:8
    for s in (1, 2, 3):
        tu = tu + np.where(j >= s, inc, NEG0)    # x + (-0.0) is x
    return tu


def _track_quotients(tu, dt, norm):
    _, off0, off1 = _constants(dt, norm)
    r = np.arange(16) & 3
    offr = np.where(r == 1, off0, np.where(r == 2, off1, NEG0))
    return _div_mu(_denorm(tu + offr, norm))


def _track_advance(tu, inc):
    for _ in range(4):
        tu = tu + inc
    return tu


def _per_step_quotients(u2, dt, norm):
    """the per-step form: lanes 8, 9, 10 of stage 0 hold u2 + (-0.0, RN(a0 k), RN(a1 k))"""
    _, off0, off1 = _constants(dt, norm)
    x = np.float64(u2) + np.array([NEG0, off0, off1])
    return _div_mu(_denorm(x, norm))


def _cases():
    """800 cases: both coordinate forms, 1..39 steps, each with its own dt, u2 at +-0, at the
    smallest denormal, negative, inside and far outside the box"""
    rng = np.random.default_rng(1305)
    edges = [0.0, -0.0, 5e-324, -5e-324, -1.0, -20.0, 500.0, -3.0e7, 1.0e9]
    out = []
    for i in range(800):
        norm = i % 2 == 0
        steps = 1 + (i // 2) % 39
        dt = 0.0025 * (1 + 0.37 * rng.integers(0, 40)) * rng.uniform(0.5, 2.0)
        u2 = edges[i % len(edges)] if i % 3 == 0 else rng.uniform(-1, 1) * 10.0 ** rng.integers(-3, 4)
        t0 = rng.uniform(0, 1)
        out.append((norm, steps, t0, t0 + steps * dt, rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), u2))
    return out


def test_final_u2_is_u2_plus_sequential_inc():
    """the oracle's u2 after `steps` RK4 steps is u2 with INC added `steps` times in sequence"""
    bad = 0
    for norm, steps, t0, t1, a, b, u2 in _cases():
        so = O.System('hopf', normalized=norm, param=(MU,))
        ref = so.rk(4, t0, t1, steps, np.array([a, b, u2]))[2]
        inc, _, _ = _constants((np.float64(t1) - np.float64(t0)) / np.float64(steps), norm)
        v = np.float64(u2)
        for _ in range(steps):
            v = v + inc
        bad += int(_bits(v)[0] != _bits(ref)[0])
    assert bad == 0, bad


def test_track_equals_the_oracle_time_component_step_by_step():
    """spread and advance: lane 4j + r of the track after p passes is the oracle's u2 after 4p + j steps"""
    rng = np.random.default_rng(1306)
    for norm in (True, False):
        so = O.System('hopf', normalized=norm, param=(MU,))
        for u2 in (0.0, -0.0, 5e-324, -0.37, 41.5, -20.0):
            dt = 0.0025 * rng.uniform(0.5, 3.0)
            inc, _, _ = _constants(dt, norm)
            tu = _track_spread(u2, inc)
            u = np.array([0.2, -0.1, u2])
            for p in range(3):
                for j in range(4):
                    n = 4 * p + j
                    # n separate one-step launches with the same dt: the kernel's h never changes
                    assert np.all(_bits(tu[4 * j:4 * j + 4]) == _bits(u[2])), (norm, u2, n)
                    u = so.rk(4, 0.0, dt, 1, u)
                tu = _track_advance(tu, inc)


def test_pass_quotients_equal_the_per_step_quotients():
    """the 12 quotients of a pass, bit for bit those the per-step form gives for the same four steps"""
    rng = np.random.default_rng(1307)
    n = 0
    for norm in (True, False):
        starts = [0.0, -0.0, 5e-324, -1.0, -20.0, 3.0e5] + list(rng.uniform(-1, 1, 20) * (1 if norm else 40))
        for u2 in starts:
            dt = 0.0025 * rng.uniform(0.5, 3.0)
            inc, _, _ = _constants(dt, norm)
            for u2s in (u2, -1.5 * inc, -2 * inc):      # the last two change sign inside the pass
                tu = _track_spread(u2s, inc)
                for p in range(2):
                    q = _track_quotients(tu, dt, norm)
                    v = tu[0]
                    for j in range(4):
                        ref = _per_step_quotients(v, dt, norm)
                        assert np.array_equal(_bits(q[4 * j:4 * j + 3]), _bits(ref)), (norm, u2s, p, j)
                        v = v + inc
                        n += 3
                    tu = _track_advance(tu, inc)
                    assert _bits(tu[0]) == _bits(v)
    assert n > 1000


def test_minus_zero_is_the_identity_of_the_masked_adds():
    x = np.array([0.0, -0.0, 5e-324, -5e-324, 1.5, -2.5, np.inf, -np.inf])
    assert np.array_equal(_bits(x + NEG0), _bits(x))


def test_fma_helper_rounds_once():
    assert _fma(1 + 2.0 ** -52, 1 + 2.0 ** -52, -1.0) == 2.0 ** -51 + 2.0 ** -104
    assert _bits(_fma(-0.0, 500.0, -0.0)) == _bits(-0.0) and _bits(_fma(0.0, 500.0, -0.0)) == _bits(0.0)
    assert _bits(_fma(3.0, 2.0, -6.0)) == _bits(0.0)
