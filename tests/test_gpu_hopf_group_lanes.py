"""The lane-group kernel's lane-batched Hopf right-hand side and its unrolled step loop
(csrc/nngp_rk_kernels.h: GroupSys<HOPF>::f_batched -- RK4 in fixed-step mode divides the time
component u2 by mu once per step, for all of the step's stage inputs, in lanes 8, 9 and 10 of each
16-lane group, from per-lane offsets set before the loop -- and rk_group_kernel's four steps per
iteration with a remainder loop) against the one-lane-per-slice kernel (NNGP_RK_GROUP=0) and, for
the '-11' system, the CPU oracle.  Compared as int64 bit patterns.

What the same-dt cases of test_gpu_hopf_group_fused.py cannot see: an offset or a quotient taken
from another slice's group (every slice has its own dt and u2 here), the remainders of the unrolled
loop (1 to 9, 12 and 13 steps, every tableau, and the group kernels without carried state), the
time component at zero of either sign, the smallest denormal and both ends of its range, and the
sampled-trajectory form, whose rows are stored between the unrolled steps."""
import numpy as np
import pytest

import oracle as O
from systems_table import oracle_ode, product_ode_norm

pytestmark = pytest.mark.gpu

SLICES = [1, 3, 4, 5, 9]
REMAINDER_STEPS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13]


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


def _slices(rng, n, steps, norm):
    """n Hopf slices, slice i with its own dt = 0.0025 (1 + 0.37 i) and its own u2"""
    U0 = rng.uniform(-0.9, 0.9, (n, 3))
    if norm:
        U0[:, :2] = rng.uniform(-0.3, 0.3, (n, 2))
        U0[:, 2] = np.linspace(-0.8, 0.7, n) if n > 1 else 0.1
    else:
        U0[:, 2] = np.linspace(-20.0, 500.0, n) if n > 1 else 37.5
    T0 = rng.uniform(0, 1, n)
    T1 = T0 + steps * 0.0025 * (1 + 0.37 * np.arange(n))
    return T0, T1, U0


@pytest.mark.parametrize('norm', [True, False], ids=['norm11', 'identity'])
@pytest.mark.parametrize('mode', ['fixed', 'linspace'])
def test_hopf_lanes_own_dt_per_slice(gpu, monkeypatch, mode, norm):
    """Every slice of a wave with another dt and another u2: k2 and the lane offsets are the
    slice's own."""
    ode = product_ode_norm(gpu, 'hopf', norm)
    rng = np.random.default_rng(11)
    for steps in (1, 5, 8):
        for n in SLICES:
            T0, T1, U0 = _slices(rng, n, steps, norm)
            assert len(set(U0[:, 2])) == n and len(set(T1 - T0)) == n
            grp, lane = _both(gpu, monkeypatch, ode, 'RK4', mode, steps, T0, T1, U0)
            assert np.all(np.isfinite(grp)), (steps, n)
            assert np.array_equal(_bits(grp), _bits(lane)), (steps, n, grp, lane)
            if norm:
                ora = _oracle('hopf', True, 'RK4', mode, steps, T0, T1, U0)
                assert np.array_equal(_bits(grp), _bits(ora)), (steps, n, grp, ora)


@pytest.mark.parametrize('name,tab', [('hopf', 'RK1'), ('hopf', 'RK2'), ('hopf', 'RK4'), ('hopf', 'RK8'),
                                      ('lorenz', 'RK4'), ('tomlab', 'RK4')])
def test_group_unrolled_loop_remainders(gpu, monkeypatch, name, tab):
    """Every remainder of the four-step (RK8: two-step) loop, with and without full iterations
    before it; Lorenz (16 lanes per slice, no carried state) and ThomasLabyrinth (4 lanes) run the
    same loop."""
    ode = product_ode_norm(gpu, name, True)
    rng = np.random.default_rng(12)
    n = 5
    for steps in REMAINDER_STEPS:
        if name == 'hopf':
            T0, T1, U0 = _slices(rng, n, steps, True)
        else:
            U0 = rng.uniform(-0.5, 0.5, (n, 3))
            T0 = rng.uniform(0, 1, n)
            T1 = T0 + steps * 0.0025 * (1 + 0.37 * np.arange(n))
        grp, lane = _both(gpu, monkeypatch, ode, tab, 'fixed', steps, T0, T1, U0)
        assert np.all(np.isfinite(grp)), steps
        assert np.array_equal(_bits(grp), _bits(lane)), (steps, grp, lane)
        ora = _oracle(name, True, tab, 'fixed', steps, T0, T1, U0)
        assert np.array_equal(_bits(grp), _bits(ora)), (steps, grp, ora)


@pytest.mark.parametrize('norm,u2', [(False, 0.0), (False, -0.0), (False, 5e-324), (False, -20.0), (False, 500.0),
                                     (True, -1.0), (True, 0.0), (True, -0.0)])
def test_hopf_lanes_time_component_edges(gpu, monkeypatch, norm, u2):
    """One slice, 1 to 5 steps: the time component at a zero of either sign (u2 + (-0.0) keeps the
    sign; u2 + k/2 and u2 + k are the reference's own additions), the smallest denormal, both ends
    of the identity system's range and the lower end of the normalised box."""
    ode = product_ode_norm(gpu, 'hopf', norm)
    T0, T1 = np.array([0.25]), np.array([0.2625])
    U0 = np.array([[0.3, -0.2, u2]])
    for mode in ('fixed', 'linspace'):
        for steps in (1, 2, 3, 4, 5):
            grp, lane = _both(gpu, monkeypatch, ode, 'RK4', mode, steps, T0, T1, U0)
            assert np.all(np.isfinite(grp)), (mode, steps)
            assert np.array_equal(_bits(grp), _bits(lane)), (mode, steps, grp, lane)
            if norm:
                ora = _oracle('hopf', True, 'RK4', mode, steps, T0, T1, U0)
                assert np.array_equal(_bits(grp), _bits(ora)), (mode, steps, grp, ora)


@pytest.mark.parametrize('norm', [True, False], ids=['norm11', 'identity'])
@pytest.mark.parametrize('tab,mode', [('RK8', 'fixed'), ('RK4', 'linspace')])
def test_hopf_unbatched_forms_still_agree(gpu, monkeypatch, tab, mode, norm):
    """RK8 and linspace RK4 keep the form that divides at every stage."""
    ode = product_ode_norm(gpu, 'hopf', norm)
    rng = np.random.default_rng(13)
    for steps in (3, 8):
        T0, T1, U0 = _slices(rng, 5, steps, norm)
        grp, lane = _both(gpu, monkeypatch, ode, tab, mode, steps, T0, T1, U0)
        assert np.all(np.isfinite(grp)), steps
        assert np.array_equal(_bits(grp), _bits(lane)), (steps, grp, lane)
        if norm:
            ora = _oracle('hopf', True, tab, mode, steps, T0, T1, U0)
            assert np.array_equal(_bits(grp), _bits(ora)), (steps, grp, ora)


@pytest.mark.parametrize('norm', [True, False], ids=['norm11', 'identity'])
@pytest.mark.parametrize('every', [1, 2, 3, 5])
def test_hopf_lanes_traj_rows(gpu, monkeypatch, every, norm):
    """Sampled trajectories: every row of the group kernel is the lane kernel's, and the last row
    is run_F_batch's end state."""
    import torch
    ode = product_ode_norm(gpu, 'hopf', norm)
    rng = np.random.default_rng(14)
    for steps in (7, 8, 9):
        T0, T1, U0 = _slices(rng, 5, steps, norm)
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
