"""Hopf on the lane-group kernel with its inline-asm right-hand side (csrc/nngp_rk.hip
GroupSys<HOPF>: one `v_fmac_f64_dpp row_newbcast` in place of a broadcast move plus an add, RK4's
third stage re-using the second's u2/mu, two steps per loop iteration and a remainder step)
against the one-lane-per-slice kernel and, for the '-11' system, the CPU oracle.  Compared as int64 bit patterns: np.array_equal cannot see a zero's sign.

Shapes: 1, 3, 4, 5, 9 slices = one 16-lane group, a partial wave, exactly one wave (4 groups),
one group and five groups past a wave boundary; 1, 2, 3 steps (the first, an even and an odd count)
and 200; every tableau (RK4 is the only one with a repeating stage) and both step modes; the
normalised ('-11', NORM = true) and the identity (NORM = false) instance."""
import numpy as np
import pytest

import oracle as O
from systems_table import oracle_system

pytestmark = pytest.mark.gpu

TABS = ['RK1', 'RK2', 'RK4', 'RK8']
STEPS = [1, 2, 3, 200]
SLICES = [1, 3, 4, 5, 9]


def _t(torch, a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _ode(gpu, norm):
    return gpu.Hopf(normalization='-11') if norm else gpu.Hopf()


def _both(gpu, monkeypatch, ode, tab, mode, steps, T0, T1, U0):
    """(group kernel result, lane kernel result) of one fine batch"""
    import torch
    s = gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=steps, F=tab, G='RK1', step_mode=mode)
    args = (_t(torch, T0), _t(torch, T1), _t(torch, U0))
    monkeypatch.setenv('NNGP_RK_GROUP', '1')
    grp = s.run_F_batch(*args).cpu().numpy()
    monkeypatch.setenv('NNGP_RK_GROUP', '0')
    lane = s.run_F_batch(*args).cpu().numpy()
    return grp, lane


def _oracle(tab, mode, steps, T0, T1, U0):
    so = oracle_system('hopf')
    m = O.STEP_FIXED if mode == 'fixed' else O.STEP_LINSPACE
    return np.array([so.rk(int(tab[2:]), T0[i], T1[i], int(steps), U0[i], m) for i in range(len(U0))])


@pytest.mark.parametrize('norm', [True, False], ids=['norm11', 'identity'])
@pytest.mark.parametrize('mode', ['fixed', 'linspace'])
@pytest.mark.parametrize('tab', TABS)
def test_hopf_group_bitwise_lane_and_oracle(gpu, monkeypatch, tab, mode, norm):
    ode = _ode(gpu, norm)
    rng = np.random.default_rng(7)
    for steps in STEPS:
        for n in SLICES:
            # identity: |u0|, |u1| < 0.9 and the time-like u2 in [-20, 500]; '-11': the normalised box,
            # u0 and u1 within +-0.3 of it (+-6.9 physical), where the explicit tableaux are stable at
            # this step (the cubic damping -3 u0^2 times h = 0.0025 stays above -0.4)
            U0 = rng.uniform(-0.9, 0.9, (n, 3))
            if norm:
                U0[:, :2] = rng.uniform(-0.3, 0.3, (n, 2))
            else:
                U0[:, 2] = rng.uniform(-20.0, 500.0, n)
            T0 = rng.uniform(0, 1, n)
            T1 = T0 + 0.0025 * steps
            grp, lane = _both(gpu, monkeypatch, ode, tab, mode, steps, T0, T1, U0)
            assert np.all(np.isfinite(grp)), (steps, n)
            assert np.array_equal(_bits(grp), _bits(lane)), (steps, n)
            if norm:
                assert np.array_equal(_bits(grp), _bits(_oracle(tab, mode, steps, T0, T1, U0))), (steps, n)


# one slice each: (u0, u1).  In the '-11' system u = 0 maps to exactly 0 ((0 + 1) * 23 - 23).
EDGES = {
    'both_zero': (0.0, 0.0),
    'u0_negzero': (-0.0, 0.0),
    'u1_negzero': (0.0, -0.0),
    'both_negzero': (-0.0, -0.0),
    'u0_zero_u1_03': (0.0, 0.3),
    'u0_03_u1_zero': (0.3, 0.0),
    'u0_denormal': (5e-324, 0.0),
    'u0_denormal_u1_03': (5e-324, 0.3),
}


@pytest.mark.parametrize('norm', [True, False], ids=['norm11', 'identity'])
@pytest.mark.parametrize('edge', list(EDGES))
def test_hopf_group_edge_states(gpu, monkeypatch, edge, norm):
    """Zeros of either sign, a zero beside a non-zero and the smallest denormal: the zero signs of
    the fused multiply-adds (q - u0^2; -+partner + x*g) are the reference additions'."""
    ode = _ode(gpu, norm)
    a, b = EDGES[edge]
    T0, T1 = np.array([0.25]), np.array([0.3])
    for tab in TABS:
        for mode in ('fixed', 'linspace'):
            for steps in (1, 2, 3):
                for u2 in ((0.0, -0.4) if norm else (0.0, -0.0, 37.5)):
                    U0 = np.array([[a, b, u2]])
                    grp, lane = _both(gpu, monkeypatch, ode, tab, mode, steps, T0, T1, U0)
                    assert np.all(np.isfinite(grp)), (tab, mode, steps, u2)
                    assert np.array_equal(_bits(grp), _bits(lane)), (tab, mode, steps, u2, grp, lane)
                    if norm:
                        ora = _oracle(tab, mode, steps, T0, T1, U0)
                        assert np.array_equal(_bits(grp), _bits(ora)), (tab, mode, steps, u2, grp, ora)


@pytest.mark.parametrize('norm', [True, False], ids=['norm11', 'identity'])
@pytest.mark.parametrize('sign', [1.0, -1.0])
def test_hopf_group_overflow(gpu, monkeypatch, sign, norm):
    """|u0| = 1e200 over 2 steps: the squares overflow.  Which NaN payload propagates is not part
    of the contract; where the non-finite values are is."""
    ode = _ode(gpu, norm)
    T0, T1 = np.array([0.25]), np.array([0.3])
    U0 = np.array([[sign * 1e200, 0.3, 0.1]])
    for tab in TABS:
        for mode in ('fixed', 'linspace'):
            grp, lane = _both(gpu, monkeypatch, ode, tab, mode, 2, T0, T1, U0)
            assert not np.all(np.isfinite(grp[:, :2])), (tab, mode)
            assert np.array_equal(np.isfinite(grp), np.isfinite(lane)), (tab, mode, grp, lane)
            assert np.array_equal(np.isnan(grp), np.isnan(lane)), (tab, mode, grp, lane)
            assert np.array_equal(grp, lane, equal_nan=True), (tab, mode, grp, lane)
            if norm:
                ora = _oracle(tab, mode, 2, T0, T1, U0)
                assert np.array_equal(grp, ora, equal_nan=True), (tab, mode, grp, ora)
