"""The device copy of csrc/nngp_math.h pinned directly, bit for bit.

Every bitwise contract of the fits, the posterior mean, the trigonometric vector fields and the
adaptive controller's powers rests on that header agreeing with the oracle's copy
(oracle/nngp_oracle.c), yet the kernels reach it only at the arguments their tests' inputs happen
to produce.  Here tests/probe/nngp_math_probe.hip -- a test-only library that includes the header
itself, built with the product's flags -- runs each routine one lane per element over the sets of
tests/math_cases.py, and the results are compared with

* the oracle's copy, for nn_exp (and its x <= 0 forms nn_exp_nonpos / nn_exp_nonpos_sep), nn_exp_dd,
  nn_pow10, nn_log, nn_sincos / nn_sin / nn_cos and nn_sin_pi: clamps and thresholds, subnormal
  results, rint ties of the reductions, quadrant edges, |n| >= 2^51, subnormal and special arguments;
* IEEE sqrt and division (numpy, float64) and the device's own sqrt() / 1.0/x, for sqrt_mid and
  rcp_mid on the whole set in_mid_range accepts and for sqrt_rcp_exact on every x > 0 -- the
  oracle's Cholesky uses sqrt and 1.0 / ljj, so correct rounding is their contract;
* the predicate in_mid_range's one compare implements, 2^-500 <= x < 2^500 (1 + 2^-20).

No tolerance anywhere: bit patterns are compared (the sign of a zero counts); where both sides are
NaN the payload is not."""
import ctypes

import numpy as np
import pytest

import math_cases as MC
import math_probe as MP
import oracle as O

pytestmark = pytest.mark.gpu

_dp = ctypes.POINTER(ctypes.c_double)


def _p(a):
    return a.ctypes.data_as(_dp)


def _oracle(fn, *args, n_out=1):
    """An orc_*_array entry point over contiguous float64 arrays."""
    args = [np.ascontiguousarray(a, dtype=np.float64) for a in args]
    outs = [np.full(args[0].shape, MP.SENTINEL) for _ in range(n_out)]
    getattr(O.lib(), fn)(args[0].size, *[_p(a) for a in args], *[_p(o) for o in outs])
    return outs[0] if n_out == 1 else outs


def _same_bits(got, want, what, *inputs):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape
    bad = (got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want))
    n = int(bad.sum())
    if n:
        i = np.flatnonzero(bad)[:8]
        rows = '; '.join(f"x={[float(v[j]).hex() for v in inputs]} got={float(got[j]).hex()} want={float(want[j]).hex()}"
                         for j in i)
        raise AssertionError(f'{what}: {n} of {got.size} elements differ in bits: {rows}')


def test_probe_refuses_bad_arguments(gpu):
    """Nothing is launched for an unknown routine, a negative count or a missing buffer."""
    import torch
    t = torch.zeros(4, dtype=torch.float64, device='cuda')
    L = MP.lib()
    assert L.nngp_math_probe(99, 4, t.data_ptr(), None, t.data_ptr(), None, None) != 0
    assert L.nngp_math_probe(0, -1, t.data_ptr(), None, t.data_ptr(), None, None) != 0
    assert L.nngp_math_probe(MP.FN['nn_exp_dd'], 4, t.data_ptr(), None, t.data_ptr(), None, None) != 0
    assert L.nngp_math_probe(MP.FN['nn_sincos'], 4, t.data_ptr(), None, t.data_ptr(), None, None) != 0
    assert L.nngp_math_probe(0, 0, None, None, None, None, None) == 0
    out, _ = MP.run('nn_exp', np.zeros(1000))      # more than one block, a partial last block
    assert np.all(out == 1.0)


def test_nn_exp_vs_oracle(gpu):
    x = MC.exp_cases()
    want = _oracle('orc_exp_array', x)
    assert np.any((want > 0) & (want < MC.DBL_MIN)) and np.any(want == np.inf) and np.any(want == 0)
    _same_bits(MP.run('nn_exp', x)[0], want, 'nn_exp', x)


@pytest.mark.parametrize('fn', ['nn_exp_nonpos', 'nn_exp_nonpos_sep'])
def test_nn_exp_nonpos_forms_vs_oracle(gpu, fn):
    x = MC.exp_nonpos_cases()
    _same_bits(MP.run(fn, x)[0], _oracle('orc_exp_array', x), fn, x)


def test_nn_exp_dd_vs_oracle(gpu):
    hi, lo = MC.exp_dd_cases()
    _same_bits(MP.run('nn_exp_dd', hi, lo)[0], _oracle('orc_exp_dd_array', hi, lo), 'nn_exp_dd', hi, lo)


def test_nn_pow10_vs_oracle(gpu):
    x = MC.pow10_cases()
    want = _oracle('orc_pow10_array', x)
    assert np.any(want == np.inf) and np.any((want == 0) & (x > -np.inf)) and np.any((want > 0) & (want < MC.DBL_MIN))
    _same_bits(MP.run('nn_pow10', x)[0], want, 'nn_pow10', x)


def test_nn_log_vs_oracle(gpu):
    x = MC.log_cases()
    _same_bits(MP.run('nn_log', x)[0], _oracle('orc_log_array', x), 'nn_log', x)


def test_nn_sincos_vs_oracle(gpu):
    x = MC.trig_cases()
    sn, cs = _oracle('orc_sincos_array', x, n_out=2)
    gs, gc = MP.run('nn_sincos', x)
    _same_bits(gs, sn, 'nn_sincos: sin', x)
    _same_bits(gc, cs, 'nn_sincos: cos', x)
    # nn_sin / nn_cos are nn_sincos's two outputs
    _same_bits(MP.run('nn_sin', x)[0], gs, 'nn_sin against nn_sincos', x)
    _same_bits(MP.run('nn_cos', x)[0], gc, 'nn_cos against nn_sincos', x)


def test_nn_sin_pi_vs_oracle(gpu):
    x = MC.trig_cases()
    _same_bits(MP.run('nn_sin_pi', x)[0], _oracle('orc_sin_pi_array', x), 'nn_sin_pi', x)


def test_in_mid_range_is_the_documented_predicate(gpu):
    x = MC.mid_range_cases()
    want = MC.mid_accepts(x)
    assert want.sum() > 1000 and (~want).sum() > 1000
    _same_bits(MP.run('in_mid_range', x)[0], want.astype(np.float64), 'in_mid_range', x)


def test_sqrt_mid_correctly_rounded_on_the_accepted_set(gpu):
    x = MC.sqrt_mid_cases()
    assert MC.mid_accepts(x).all()
    got, dev = MP.run('sqrt_mid', x)
    want = np.sqrt(x)
    _same_bits(dev, want, "the device's sqrt against IEEE", x)
    _same_bits(got, want, 'sqrt_mid against IEEE', x)
    _same_bits(got, dev, "sqrt_mid against the device's sqrt", x)


def test_rcp_mid_correctly_rounded_on_the_accepted_set(gpu):
    x = MC.rcp_mid_cases()
    assert MC.mid_accepts(x).all()
    got, dev = MP.run('rcp_mid', x)
    want = 1.0 / x
    _same_bits(dev, want, "the device's 1.0 / x against IEEE", x)
    _same_bits(got, want, 'rcp_mid against IEEE', x)
    _same_bits(got, dev, "rcp_mid against the device's 1.0 / x", x)


def test_sqrt_rcp_exact_every_positive_x(gpu):
    x = MC.sqrt_rcp_cases()
    ljj, ri = MP.run('sqrt_rcp_exact', x)
    s = np.sqrt(x)
    _same_bits(ljj, s, 'sqrt_rcp_exact: sqrt', x)
    _same_bits(ri, 1.0 / s, 'sqrt_rcp_exact: reciprocal', x)
    assert ljj[-1] == np.inf and ri[-1] == 0 and not np.signbit(ri[-1])    # +inf -> (inf, +0)
