"""The arithmetic the lane-group kernel's folded tableau rests on (csrc/nngp_rk_dev.h, fold_*), in
numpy on the host: a stage's k is stored pre-scaled by the tableau's power-of-two entry,
k' = (a h) o in place of a (h o), and every other coefficient on that column is divided by a.

Scaling by a power of two commutes with rounding while the products are normal, so both are the
same doubles bit for bit; where h o is subnormal they can differ in the last denormal bit, the
documented limit, pinned here by one explicit example."""
import numpy as np

N = 1_000_000
TINY = np.finfo(np.float64).tiny   # smallest normal


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _wide(rng, n):
    """doubles of either sign over 200 decades"""
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-100, 100, n)


def _normal_pairs(rng, a):
    h, o = _wide(rng, N), _wide(rng, N)
    with np.errstate(over='ignore', under='ignore'):
        p = np.abs(h * o)
    ok = (np.abs(a * h) >= TINY) & (p * a >= 4 * TINY) & np.isfinite(p) & (h != 0) & (o != 0)
    assert ok.sum() > 0.9 * N
    return h[ok], o[ok]


def test_power_of_two_scale_commutes_with_rounding_for_normal_products():
    rng = np.random.default_rng(9)
    for a in (0.5, 0.25):
        h, o = _normal_pairs(rng, a)
        assert np.array_equal(_bits(a * (h * o)), _bits((a * h) * o)), a


def test_step_sized_pairs():
    """the magnitudes the propagators run at: h of a fine step, o of a normalised field"""
    rng = np.random.default_rng(10)
    h = 10.0 ** rng.uniform(-9, 0, N)
    o = rng.standard_normal(N) * 10.0 ** rng.uniform(-12, 6, N)
    for a in (0.5, 0.25):
        assert np.array_equal(_bits(a * (h * o)), _bits((a * h) * o)), a


def test_signed_zeros_keep_their_sign():
    h = np.array([0.0025, 0.0025, -0.0025, -0.0025])
    o = np.array([0.0, -0.0, 0.0, -0.0])
    for a in (0.5, 0.25):
        assert np.array_equal(_bits(a * (h * o)), _bits((a * h) * o))
    assert np.array_equal(np.signbit(0.5 * h * o), [False, True, True, False])


def test_rescaled_update_coefficients():
    """column j scaled by a: the update's b k becomes (b / a) k' with k' = a k, the same product"""
    rng = np.random.default_rng(11)
    k = _wide(rng, N)
    k = k[np.abs(k) >= 8 * TINY]
    b8 = float.fromhex('0x1.999999999999ap-5')   # RK8's B[0]
    a83 = float.fromhex('0x1.2492492492492p-3')  # RK8's A[3][0]
    for b in (1.0 / 6, 1.0 / 3, b8, a83, 0.25):
        assert b / 0.5 == 2 * b and (2 * b) / 2 == b      # the rescaling itself is exact
        assert np.array_equal(_bits((2 * b) * (k / 2)), _bits(b * k)), b
        assert np.array_equal(_bits((4 * b) * (k / 4)), _bits(b * k)), b
    # RK4's folded weights are the doubles 1/3, 2/3, 1/3, 1/6
    assert 2 * (1.0 / 6) == 1.0 / 3 and 2 * (1.0 / 3) == 2.0 / 3


def test_subnormal_products_can_differ_in_the_last_bit():
    """The limit, not a property to fix: h o = 2.75 units of 2^-1074 rounds to 3 units and its half
    (a tie) to 2, while (h/2) o = 1.375 units rounds to 1."""
    h, o = np.float64(11 * 2.0 ** -538), np.float64(2.0 ** -538)
    assert abs(h) >= TINY and abs(o) >= TINY and abs(0.5 * h) >= TINY
    two_step = 0.5 * (h * o)
    folded = (0.5 * h) * o
    unit = np.float64(5e-324)
    assert h * o == 3 * unit
    assert two_step == 2 * unit and folded == unit
    assert _bits(two_step) != _bits(folded)
