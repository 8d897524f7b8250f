"""The Hopf group kernel's pass statement (csrc/nngp_rk_kernels.h: GroupSys<HOPF>::pass_asm, the
sixteen-step loop of rk_group_kernel's TRACK form: RK4, fixed-step mode, normalised coordinates)
against the one-lane-per-slice kernel (NNGP_RK_GROUP=0) and, for the normalised system, the CPU
oracle.  Compared as int64 bit patterns.

The long loop runs four steps as one asm statement in an order of its own, fifteen of its sixteen
stages with both subtractions of g fused, and alternates the quotient register from pass to pass;
the remainder (a four-step loop, then up to three steps), the sampled-trajectory form and the
identity coordinates keep the statement-per-stage form.  So the cases walk every remainder behind
none, one, two and three iterations of the long loop, partial waves, a time component that is zero,
denormal, far outside the box or changes sign inside a pass of the long loop, zeros and an exact
cancellation in g, and pin that the end state is the sampled-trajectory form's last row and that
the forms the statement does not apply to still equal the lane kernel."""
import numpy as np
import pytest

import oracle as O
from systems_table import oracle_ode, product_ode_norm

pytestmark = pytest.mark.gpu

STEPS = list(range(1, 10)) + [15, 16, 17, 19, 20, 31, 32, 33, 35, 48, 49]
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
    """Every remainder of the pass and of the sixteen-step loop, with none, one, two and three full
    iterations in front; 5 slices, each with its own dt."""
    rng = np.random.default_rng(41)
    for steps in STEPS:
        U0 = _states('hopf', norm, 5, rng)
        T0, T1 = _own_dt(rng, 5, steps)
        _check(gpu, monkeypatch, 'hopf', norm, 'RK4', 'fixed', steps, T0, T1, U0)


@NORMS
@pytest.mark.parametrize('n', SLICES)
def test_slice_counts(gpu, monkeypatch, n, norm):
    """partial waves: a wave holds four slices"""
    rng = np.random.default_rng(42)
    for steps in (16, 17, 32, 35):
        U0 = _states('hopf', norm, n, rng)
        T0, T1 = _own_dt(rng, n, steps)
        _check(gpu, monkeypatch, 'hopf', norm, 'RK4', 'fixed', steps, T0, T1, U0)


@NORMS
@pytest.mark.parametrize('mult', [-1.5, -2.0, -9.5, -21.5])
def test_u2_changes_sign_inside_a_pass(gpu, monkeypatch, mult, norm):
    """One slice whose time component starts at mult * INC (in the kernel's coordinates): it
    passes through zero, or onto it, inside the first pass of the long loop (-1.5, -2), its third
    (-9.5) and the second of the second iteration (-21.5, at 32 and 33 steps)."""
    T0 = np.array([0.25])
    for steps in (16, 17, 32, 33):
        T1 = T0 + steps * 0.0025
        u2 = mult * _inc(T0[0], T1[0], steps, norm)
        U0 = np.array([[0.3, -0.2, u2]]) if norm else np.array([[6.9, -4.6, u2]])
        _check(gpu, monkeypatch, 'hopf', norm, 'RK4', 'fixed', steps, T0, T1, U0)


@pytest.mark.parametrize('norm,u2', [(False, 0.0), (False, -0.0), (False, 5e-324), (False, -20.0), (False, 3.0e4),
                                     (True, -1.0), (True, 0.0), (True, -0.0), (True, 5e-324), (True, 4.0e4),
                                     (True, -3.0e4)])
def test_u2_edges(gpu, monkeypatch, norm, u2):
    """One slice: the time component at a zero of either sign, the smallest denormal, the identity
    system's start, the lower end of the normalised box and far outside the box."""
    T0 = np.array([0.25])
    U0 = np.array([[0.3, -0.2, u2]])
    for steps in (16, 17, 32, 33):
        _check(gpu, monkeypatch, 'hopf', norm, 'RK4', 'fixed', steps, T0, T0 + steps * 0.0025, U0)


@pytest.mark.parametrize('s0,s1', [(0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0)])
def test_zeros_in_every_stage(gpu, monkeypatch, s0, s1):
    """Hopf at its equilibrium u0 = u1 = +-0 (identity coordinates, where the zeros reach the field
    as they are): the zeros come out as zeros with the lane kernel's signs."""
    T0 = np.array([0.25])
    U0 = np.array([[s0, s1, 37.5]])
    for steps in (16, 17, 32):
        grp = _check(gpu, monkeypatch, 'hopf', False, 'RK4', 'fixed', steps, T0, T0 + steps * 0.0025, U0)
        assert np.all(grp[0, :2] == 0.0), (steps, grp)


@pytest.mark.parametrize('u0,u1', [(3.0, 4.0), (-3.0, 4.0), (4.0, -3.0)])
def test_exact_cancellation_in_g(gpu, monkeypatch, u0, u1):
    """One slice in identity coordinates with u2 = mu (u0^2 + u1^2) and exactly representable
    squares: u2/mu = 25, so (q - u0^2) - u1^2 is an exact zero at stage 0 of the first step; its sign
    and everything after it equal the lane kernel's."""
    ode = product_ode_norm(gpu, 'hopf', False)
    mu = float(ode.param[0])
    u2 = 25.0 * mu
    assert u2 / 25.0 == mu and u2 / mu == 25.0   # 25 mu is exact, and so is the correctly rounded quotient
    T0 = np.array([0.0])
    U0 = np.array([[u0, u1, u2]])
    for steps in (1, 4, 16, 17, 32):
        _check(gpu, monkeypatch, 'hopf', False, 'RK4', 'fixed', steps, T0, T0 + steps * 0.0025, U0)


@NORMS
@pytest.mark.parametrize('every', [1, 3])
def test_end_state_is_last_traj_row(gpu, monkeypatch, every, norm):
    """The long loop of run_F_batch runs the pass statement and the sampled-trajectory form the
    statement-per-stage one: the end state of the former is the last row of the latter."""
    import torch
    ode = product_ode_norm(gpu, 'hopf', norm)
    rng = np.random.default_rng(44)
    monkeypatch.setenv('NNGP_RK_GROUP', '1')
    for steps in (16, 17, 33):
        U0 = _states('hopf', norm, 5, rng)
        T0, T1 = _own_dt(rng, 5, steps)
        s = _solver(gpu, ode, 'RK4', 'fixed', steps)
        args = (_t(torch, T0), _t(torch, T1), _t(torch, U0))
        traj = s.run_F_traj_batch(*args, every=every).cpu().numpy()
        end = s.run_F_batch(*args).cpu().numpy()
        assert traj.shape == (5, s.traj_rows(steps, every), 3)
        assert np.all(np.isfinite(end)), steps
        assert np.array_equal(_bits(traj[:, -1]), _bits(end)), (steps, traj[:, -1], end)


@NORMS
@pytest.mark.parametrize('name,tab,mode', [('hopf', 'RK1', 'fixed'), ('hopf', 'RK2', 'fixed'),
                                           ('hopf', 'RK8', 'fixed'), ('hopf', 'RK4', 'linspace'),
                                           ('lorenz', 'RK4', 'fixed')])
def test_unchanged_forms(gpu, monkeypatch, name, tab, mode, norm):
    """the tableaux, the step mode and the systems the statement does not apply to still equal the lane kernel"""
    rng = np.random.default_rng(45)
    for steps in (1, 4, 16, 17):
        U0 = _states(name, norm, 5, rng)
        T0, T1 = _own_dt(rng, 5, steps)
        _check(gpu, monkeypatch, name, norm, tab, mode, steps, T0, T1, U0)
