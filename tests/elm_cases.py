"""The two whole runs the ELM tests share (Lorenz N = 32 and FHN-ODE N = 40 at the ELM defaults,
'-11' normalisation, eps = 5e-7): the restatement's loop (tests/elm_ref.py), computed once per
session and left unchanged, and the serial fine solution at the slice boundaries.  Not a test
module."""
import numpy as np

import elm_ref as E
import oracle as O

# name -> (oracle system, tspan, N, Ng, Nf, G); F = RK4
RUNS = {'lorenz': ('lorenz', [0, 18], 32, 6, 450, 'RK4'), 'fhn_ode': ('fhn_ode', [0, 40], 40, 4, 400, 'RK2')}
EPS = 5e-7


def run_cfg(name):
    """(oracle system, u0, args of elm_ref.parareal_elm) of one of the two whole runs."""
    sysname, tspan, N, Ng, Nf, G = RUNS[name]
    so = O.System(sysname)
    return so, so.fit(O.BOUNDS[sysname][2]), (tspan, N, Ng, Nf, G, 'RK4')


_loops = {}


def cpu_loop(name, tau=E.TAU):
    """The restatement's whole run at the threshold tau (the model's by default), computed once per
    session and left unchanged."""
    if (name, tau) not in _loops:
        so, u0, args = run_cfg(name)
        r = E.parareal_elm(so, *args, epsilon=EPS, u0=u0, tau=tau)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _loops[name, tau] = r
    return _loops[name, tau]


def serial_fine(name):
    so, u0, (tspan, N, Ng, Nf, G, F) = run_cfg(name)
    t = np.linspace(tspan[0], tspan[1], N + 1)
    f = [u0]
    for i in range(N):
        f.append(so.rk(4, t[i], t[i + 1], Nf, f[-1]))
    return np.array(f)
