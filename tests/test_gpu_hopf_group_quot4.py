"""The Hopf group kernel's time track (csrc/nngp_rk_kernels.h: GroupSys<HOPF>::track_div / f_take,
rk_group_kernel's TRACK form: RK4 in fixed-step mode) against the one-lane-per-slice kernel
(NNGP_RK_GROUP=0) and, for the normalised system, the CPU oracle.  Compared as int64 bit patterns.

The track holds the u2/mu quotients of four steps at once (a pass), and inside a pass the second
stage of the first steps carries two instructions of the next pass's division between its two fused
subtractions (f_take2), so the cases walk every
remainder of the four-step pass and of the sixteen-step loop, partial waves, a time component that
is zero, denormal, far outside the box or changes sign inside a pass, and the sampled-trajectory
form; the forms the track does not apply to are pinned as unchanged.  The host side of the argument
is tests/test_hopf_time_track_host.py."""
import numpy as np
import pytest

import oracle as O
from systems_table import oracle_ode, product_ode_norm

pytestmark = pytest.mark.gpu

STEPS = list(range(1, 10)) + [13, 15, 16, 17, 19, 20, 33, 35]
SLICES = [1, 3, 4, 5, 9]
NORMS = pytest.mark.parametrize('norm', [True, False], ids=['norm11', 'identity'])


def _t(torch, a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _solver(gpu, ode, tab, mode, steps):
    return gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=steps, F=tab, G='RK1', step_mode=mode)


def _both(gpu, monkeypatch, ode, tab, mode, steps, T0, T1, U0):
    """(group kernel result, lane kernel result) of one fine batch"""
    import torch
    s = _solver(gpu, ode, tab, mode, steps)
    args = (_t(torch, T0), _t(torch, T1), _t(torch, U0))
    monkeypatch.setenv('NNGP_RK_GROUP', '1')
    grp = s.run_F_batch(*args).cpu().numpy()
    monkeypatch.setenv('NNGP_RK_GROUP', '0')
    lane = s.run_F_batch(*args).cpu().numpy()
    return grp, lane


def _check(gpu, monkeypatch, name, norm, tab, mode, steps, T0, T1, U0):
    ode = product_ode_norm(gpu, name, norm)
    grp, lane = _both(gpu, monkeypatch, ode, tab, mode, steps, T0, T1, U0)
    at = (name, norm, tab, mode, steps, len(U0))
    assert np.all(np.isfinite(grp)), at
    assert np.array_equal(_bits(grp), _bits(lane)), (at, grp, lane)
    if norm:
        so = oracle_ode(name, True)
        m = O.STEP_FIXED if mode == 'fixed' else O.STEP_LINSPACE
        ora = np.array([so.rk(int(tab[2:]), T0[i], T1[i], int(steps), U0[i], m) for i in range(len(U0))])
        assert np.array_equal(_bits(grp), _bits(ora)), (at, grp, ora)
    return grp


def _states(name, norm, n, rng):
    """uniform in +-0.3 of the normalised box; identity: the same draws in the physical box"""
    u = rng.uniform(-0.3, 0.3, (n, len(O.BOUNDS[name][0])))
    if not norm:
        mn, mx = (np.asarray(b, dtype=float) for b in O.BOUNDS[name][:2])
        u = mn + (u + 1) / 2 * (mx - mn)
    return u


def _own_dt(rng, n, steps):
    """slice i with its own dt = 0.0025 (1 + 0.37 i)"""
    T0 = rng.uniform(0, 1, n)
    return T0, T0 + steps * 0.0025 * (1 + 0.37 * np.arange(n))


def _inc(T0, T1, steps, norm):
    """what one RK4 step adds to u2, from the kernel's own expressions (folded tableau)"""
    dt = (np.float64(T1) - np.float64(T0)) / np.float64(steps)
    mn, mx = O.BOUNDS['hopf'][0][2], O.BOUNDS['hopf'][1][2]
    o = np.float64(1.0) * (2 / (np.float64(mx) - mn)) if norm else np.float64(1.0)
    k01, k23 = (0.5 * dt) * o, dt * o
    return (((1.0 / 3) * k01 + (2.0 / 3) * k01) + (1.0 / 3) * k23) + (1.0 / 6) * k23


@NORMS
def test_step_counts(gpu, monkeypatch, norm):
    """Every remainder of the four-step pass and of the sixteen-step loop, with none, one and two
    full iterations before it; 5 slices, each with its own dt."""
    rng = np.random.default_rng(31)
    for steps in STEPS:
        U0 = _states('hopf', norm, 5, rng)
        T0, T1 = _own_dt(rng, 5, steps)
        _check(gpu, monkeypatch, 'hopf', norm, 'RK4', 'fixed', steps, T0, T1, U0)


@NORMS
@pytest.mark.parametrize('n', SLICES)
def test_slice_counts(gpu, monkeypatch, n, norm):
    """partial waves: a wave holds four slices"""
    rng = np.random.default_rng(32)
    for steps in (3, 4, 17, 35):
        U0 = _states('hopf', norm, n, rng)
        T0, T1 = _own_dt(rng, n, steps)
        _check(gpu, monkeypatch, 'hopf', norm, 'RK4', 'fixed', steps, T0, T1, U0)


@NORMS
@pytest.mark.parametrize('mult', [-1.5, -2.0, -9.5])
def test_u2_changes_sign_inside_a_pass(gpu, monkeypatch, mult, norm):
    """One slice whose time component starts at mult * INC (in the kernel's coordinates): it
    passes through zero, or onto it, inside the first pass (-1.5, -2) and inside the third (-9.5)."""
    T0 = np.array([0.25])
    for steps in (1, 2, 3, 4, 5, 8, 12, 17):
        T1 = T0 + steps * 0.0025
        u2 = mult * _inc(T0[0], T1[0], steps, norm)
        U0 = np.array([[0.3, -0.2, u2]]) if norm else np.array([[6.9, -4.6, u2]])
        _check(gpu, monkeypatch, 'hopf', norm, 'RK4', 'fixed', steps, T0, T1, U0)


@pytest.mark.parametrize('norm,u2', [(False, 0.0), (False, -0.0), (False, 5e-324), (False, -20.0),
                                     (True, -1.0), (True, 0.0), (True, -0.0), (True, 4.0e4), (True, -3.0e4)])
def test_u2_edges(gpu, monkeypatch, norm, u2):
    """One slice: the time component at a zero of either sign, the smallest denormal, the identity
    system's start, the lower end of the normalised box and far outside it."""
    T0 = np.array([0.25])
    U0 = np.array([[0.3, -0.2, u2]])
    for steps in (1, 2, 3, 4, 5, 9, 16, 17, 20):
        _check(gpu, monkeypatch, 'hopf', norm, 'RK4', 'fixed', steps, T0, T0 + steps * 0.0025, U0)


@pytest.mark.parametrize('s0,s1', [(0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0)])
def test_zeros_keep_their_sign(gpu, monkeypatch, s0, s1):
    """Hopf at its equilibrium u0 = u1 = +-0 (identity coordinates, where the zeros reach the field
    as they are): every stage is a take stage now, and the zeros must pass through it with their signs."""
    T0 = np.array([0.25])
    U0 = np.array([[s0, s1, 37.5]])
    for steps in (1, 2, 3, 4, 5, 17):
        grp = _check(gpu, monkeypatch, 'hopf', False, 'RK4', 'fixed', steps, T0, T0 + steps * 0.0025, U0)
        assert np.all(grp[0, :2] == 0.0), (steps, grp)
    for steps in (1, 4, 5):   # the same through the '-11' wrapper, against the oracle as well
        _check(gpu, monkeypatch, 'hopf', True, 'RK4', 'fixed', steps, T0, T0 + steps * 0.0025,
               np.array([[s0, s1, 0.1]]))


@NORMS
@pytest.mark.parametrize('every', [1, 2, 3, 5])
def test_traj_rows(gpu, monkeypatch, every, norm):
    """Sampled trajectories: the rows are stored between the steps of a pass; every row of the group
    kernel is the lane kernel's, and the last row is run_F_batch's end state."""
    import torch
    ode = product_ode_norm(gpu, 'hopf', norm)
    rng = np.random.default_rng(34)
    for steps in (15, 16, 17, 33):
        U0 = _states('hopf', norm, 5, rng)
        T0, T1 = _own_dt(rng, 5, steps)
        s = _solver(gpu, ode, 'RK4', 'fixed', steps)
        args = (_t(torch, T0), _t(torch, T1), _t(torch, U0))
        monkeypatch.setenv('NNGP_RK_GROUP', '1')
        grp = s.run_F_traj_batch(*args, every=every).cpu().numpy()
        end = s.run_F_batch(*args).cpu().numpy()
        monkeypatch.setenv('NNGP_RK_GROUP', '0')
        lane = s.run_F_traj_batch(*args, every=every).cpu().numpy()
        assert grp.shape == (5, s.traj_rows(steps, every), 3)
        assert np.all(np.isfinite(grp)), steps
        assert np.array_equal(_bits(grp), _bits(lane)), (steps, grp, lane)
        assert np.array_equal(_bits(grp[:, -1]), _bits(end)), (steps, grp[:, -1], end)
        assert np.array_equal(_bits(grp[:, 0]), _bits(U0)), steps


@NORMS
@pytest.mark.parametrize('name,tab,mode', [('hopf', 'RK1', 'fixed'), ('hopf', 'RK2', 'fixed'),
                                           ('hopf', 'RK8', 'fixed'), ('hopf', 'RK4', 'linspace'),
                                           ('lorenz', 'RK4', 'fixed')])
def test_unchanged_forms(gpu, monkeypatch, name, tab, mode, norm):
    """the tableaux, the step mode and the systems the track does not apply to still equal the lane kernel"""
    rng = np.random.default_rng(35)
    for steps in (1, 4, 16, 17):
        U0 = _states(name, norm, 5, rng)
        T0, T1 = _own_dt(rng, 5, steps)
        _check(gpu, monkeypatch, name, norm, tab, mode, steps, T0, T1, U0)
