"""CPU: the host side of the sampled-trajectory launch (include/nngp.h nngp_rk_traj): the row count
and time stamps SolverRK derives from (steps, every), the argument checks the C entry makes before
it touches the GPU, and Parareal.build_cont_traj's demand for a key when there are several runs."""
import ctypes

import numpy as np
import pytest


@pytest.mark.parametrize('steps,every,rows', [(1, 1, 2), (6, 3, 3), (8, 3, 4), (3, 5, 2)])
def test_traj_rows(steps, every, rows):
    import nngp_amd
    assert nngp_amd.SolverRK.traj_rows(steps, every) == rows


def test_traj_times_are_the_linspace_points_of_the_sampled_steps():
    import nngp_amd
    got = nngp_amd.SolverRK.traj_times(0, 1, 8, 3)
    assert np.array_equal(got, np.linspace(0, 1, 9)[[0, 3, 6, 8]])
    # every row count of traj_rows has its time stamp, the last one t1 itself
    for steps, every in [(1, 1), (6, 3), (7, 2), (3, 5)]:
        t = nngp_amd.SolverRK.traj_times(0.25, 0.75, steps, every)
        assert len(t) == nngp_amd.SolverRK.traj_rows(steps, every) and t[0] == 0.25 and t[-1] == 0.75


def test_rk_traj_argument_errors_are_reported_without_a_gpu():
    import nngp_amd
    L = nngp_amd.lib()
    cs = nngp_amd._lib.CSystem(0, 3, 0, 0, (ctypes.c_double * 4)(), None)
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # (sys, tableau, step_mode, n_slices, t0, t1, steps, every, u0, traj, stream)
    assert L.nngp_rk_traj(None, 4, 0, 1, p, p, 8, 1, p, p, None) == -1
    assert b'sys is NULL' in L.nngp_last_error()
    assert L.nngp_rk_traj(ctypes.byref(cs), 4, 0, 1, p, p, 8, 0, p, p, None) == -1
    assert b'every' in L.nngp_last_error()
    assert L.nngp_rk_traj(ctypes.byref(cs), 4, 0, 1, p, p, 0, 1, p, p, None) == -1
    assert b'steps' in L.nngp_last_error()
    assert L.nngp_rk_traj(ctypes.byref(cs), 4, 0, 1, p, p, 8, 1, p, None, None) == -1
    assert b'null array' in L.nngp_last_error()
    assert L.nngp_rk_traj(ctypes.byref(cs), 4, 0, 1, p, p, 8, 1, None, p, None) == -1
    assert L.nngp_rk_traj(ctypes.byref(cs), 4, 7, 1, p, p, 8, 1, p, p, None) == -1
    assert b'step_mode' in L.nngp_last_error()
    assert L.nngp_rk_traj(ctypes.byref(cs), 4, 0, -1, p, p, 8, 1, p, p, None) == -1
    assert L.nngp_rk_traj(ctypes.byref(cs), 4, 0, 0, None, None, 8, 1, None, None, None) == 0   # empty batch
    assert L.nngp_rk_traj(ctypes.byref(cs), 4, 1 | 16, 0, None, None, 8, 3, None, None, None) == 0


def test_build_cont_traj_needs_a_key_when_there_are_several_runs():
    import nngp_amd
    ode = nngp_amd.Lorenz(normalization='-11')
    s = nngp_amd.SolverRK(ode.get_vector_field(), Ng=6, Nf=45, F='RK4', G='RK4')
    p = nngp_amd.Parareal(ode, s, [0, 4], 8, verbose=None)
    p.runs['a'] = {'t': np.linspace(0, 4, 9), 'u': np.zeros((9, 3, 1))}
    p.runs['b'] = {'t': np.linspace(0, 4, 9), 'u': np.zeros((9, 3, 1))}
    with pytest.raises(Exception, match='Multiple runs, must specify key'):
        p.build_cont_traj()
    p.runs = {}   # and with none at all
    with pytest.raises(Exception, match='Multiple runs, must specify key'):
        p.build_cont_traj()


def test_traj_batch_rejects_every_below_one():
    import nngp_amd
    ode = nngp_amd.Lorenz(normalization='-11')
    s = nngp_amd.SolverRK(ode.get_vector_field(), Ng=6, Nf=45, F='RK4', G='RK4')

    class _U:   # the check comes before any tensor is touched
        shape = (1, 3)
    with pytest.raises(ValueError, match='every'):
        s.run_F_traj_batch(None, None, _U(), every=0)
