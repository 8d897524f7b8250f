"""The lane-group kernel's folded tableau and its deeper unrolled loop (csrc/nngp_rk_dev.h: fold_*;
csrc/nngp_rk_kernels.h: rk_group_kernel) against the one-lane-per-slice kernel (NNGP_RK_GROUP=0)
and, for the '-11' systems, the CPU oracle.  Compared as int64 bit patterns.

The fold stores a stage's k pre-scaled by the tableau's power-of-two entry (RK2, RK4 and RK8 each
have one on k0, RK4 a second on k1) and rescales every other coefficient on that column, in every
group kernel; U is the number of steps per loop iteration for the tableaux of up to four stages
(RK8: two).  The host side of the argument is tests/test_half_step_fold_host.py."""
import numpy as np
import pytest

import oracle as O
from systems_table import ODE_SYSTEMS, oracle_ode, product_ode_norm

pytestmark = pytest.mark.gpu

U = 16
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


def _oracle(name, norm, tab, mode, steps, T0, T1, U0):
    so = oracle_ode(name, norm)
    m = O.STEP_FIXED if mode == 'fixed' else O.STEP_LINSPACE
    return np.array([so.rk(int(tab[2:]), T0[i], T1[i], int(steps), U0[i], m) for i in range(len(U0))])


def _check(gpu, monkeypatch, name, norm, tab, mode, steps, T0, T1, U0):
    ode = product_ode_norm(gpu, name, norm)
    grp, lane = _both(gpu, monkeypatch, ode, tab, mode, steps, T0, T1, U0)
    at = (name, norm, tab, mode, steps, len(U0))
    assert np.all(np.isfinite(grp)), at
    assert np.array_equal(_bits(grp), _bits(lane)), (at, grp, lane)
    if norm:
        ora = _oracle(name, True, tab, mode, steps, T0, T1, U0)
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


@pytest.mark.parametrize('name,tab', [('hopf', 'RK1'), ('hopf', 'RK2'), ('hopf', 'RK4'), ('hopf', 'RK8'),
                                      ('lorenz', 'RK4'), ('tomlab', 'RK4')])
def test_loop_remainders(gpu, monkeypatch, name, tab):
    """Every remainder of the U-step loop with none, one and two full iterations before it, and
    one step past three; 5 slices, each with its own dt."""
    rng = np.random.default_rng(21)
    for steps in list(range(1, 2 * U + 2)) + [3 * U + 1]:
        U0 = _states(name, True, 5, rng)
        T0, T1 = _own_dt(rng, 5, steps)
        _check(gpu, monkeypatch, name, True, tab, 'fixed', steps, T0, T1, U0)


@NORMS
@pytest.mark.parametrize('tab', ['RK2', 'RK4', 'RK8'])
@pytest.mark.parametrize('name', list(ODE_SYSTEMS))
def test_fold_every_group_system(gpu, monkeypatch, name, tab, norm):
    """Every system with a group kernel, every tableau with a folded column, both step modes and
    both coordinate forms; partial waves; the first steps and both sides of the loop's edge."""
    rng = np.random.default_rng(22)
    for mode in ('fixed', 'linspace'):
        for steps in (1, 2, U, U + 1):
            for n in SLICES:
                U0 = _states(name, norm, n, rng)
                T0, T1 = _own_dt(rng, n, steps)
                _check(gpu, monkeypatch, name, norm, tab, mode, steps, T0, T1, U0)


@pytest.mark.parametrize('tab', ['RK1', 'RK2', 'RK4', 'RK8'])
@pytest.mark.parametrize('s0,s1', [(0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0)])
def test_hopf_zeros_keep_their_sign(gpu, monkeypatch, s0, s1, tab):
    """Hopf at its equilibrium u0 = u1 = +-0 (identity coordinates, where the zeros reach the field
    as they are): every k of those components is a zero whose sign must pass through k' and the
    rescaled update as it passes through k in the lane kernel."""
    T0, T1 = np.array([0.25]), np.array([0.2625])
    U0 = np.array([[s0, s1, 37.5]])
    for mode in ('fixed', 'linspace'):
        for steps in (1, 2, 3, 4, 5):
            grp = _check(gpu, monkeypatch, 'hopf', False, tab, mode, steps, T0, T1, U0)
            assert np.all(grp[0, :2] == 0.0), (mode, steps, grp)


@pytest.mark.parametrize('tab', ['RK2', 'RK4'])
def test_hopf_zeros_normalised(gpu, monkeypatch, tab):
    """The same equilibrium through the '-11' wrapper (u = +-0 de-normalises to the box centre),
    against the oracle as well."""
    T0, T1 = np.array([0.25]), np.array([0.2625])
    for s0, s1 in ((0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0)):
        U0 = np.array([[s0, s1, 0.1]])
        for steps in (1, 2, 3, 4, 5):
            _check(gpu, monkeypatch, 'hopf', True, tab, 'fixed', steps, T0, T1, U0)


@pytest.mark.parametrize('tab', ['RK2', 'RK4', 'RK8'])
@pytest.mark.parametrize('norm,u2', [(False, 0.0), (False, -0.0), (False, 5e-324), (False, -20.0), (False, 500.0),
                                     (True, -1.0), (True, 0.0), (True, -0.0)])
def test_hopf_time_component_edges(gpu, monkeypatch, norm, u2, tab):
    """One slice: the time component at a zero of either sign, the smallest denormal, both ends of
    the identity system's range and the lower end of the normalised box, for the folded forms."""
    T0, T1 = np.array([0.25]), np.array([0.2625])
    U0 = np.array([[0.3, -0.2, u2]])
    for mode in ('fixed', 'linspace'):
        for steps in (1, 2, 3, 4, 5, U, U + 1):
            _check(gpu, monkeypatch, 'hopf', norm, tab, mode, steps, T0, T1, U0)


@NORMS
@pytest.mark.parametrize('every', [1, 2, 3, 5])
def test_hopf_traj_rows(gpu, monkeypatch, every, norm):
    """Sampled trajectories: the rows are stored between the unrolled steps; every row of the group
    kernel is the lane kernel's, and the last row is run_F_batch's end state."""
    import torch
    ode = product_ode_norm(gpu, 'hopf', norm)
    rng = np.random.default_rng(24)
    for steps in (U - 1, U, U + 1, 2 * U + 1):
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
