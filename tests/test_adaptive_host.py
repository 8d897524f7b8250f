"""CPU: the adaptive propagator's contract and surface without a GPU.

* tests/adaptive_ref.py (the normative restatement) against the reference's own
  SolverScipy.run_F and a direct solve_ivp call, recorded in tests/golden/adaptive.npz: the same
  number of evaluations and accepted steps on every case, the end state within BOUND.
  BOUND is ten times the largest relative deviation measured over the fixture when it was
  generated (2.855e-14, printed by tests/golden/gen_adaptive.py): the margin is for another libm or
  BLAS under scipy; a step-count flip would show as 1e-6 or worse.
* the sum order of the error norm on hand-computed cases;
* SolverScipy's Python surface and nngp_rk_adaptive's argument checks, neither touching the GPU."""
import ctypes
import warnings

import numpy as np
import pytest

import adaptive_ref as AR
import oracle as O
from conftest import golden
from diffreact_ref import DiffReactNP

BOUND = 10 * 2.855e-14

FIELDS = {
    'lorenz': lambda: O.System('lorenz').rhs,
    'lorenz_id': lambda: O.System('lorenz', normalized=False).rhs,
    'fhn_ode': lambda: O.System('fhn_ode').rhs,
    'brus': lambda: O.System('brus').rhs,
    'tomlab': lambda: O.System('tomlab').rhs,
    'burgers16': lambda: O.System('burgers', d=16, param=(0.01,), mn=0, mx=1).rhs,
    'fhnpde4': lambda: O.System('fhn_pde', nx=4, normalized=False).rhs,
    'diffreact3': lambda: DiffReactNP(3),
}
KEYS = [f'{s}__{m}__{c}' for s in FIELDS for m in ('RK23', 'RK45') for c in ('max', 'rej', 'clip')]


def test_fixture_holds_every_system_method_and_class():
    g = golden('adaptive.npz')
    assert sorted(g['keys'].tolist()) == sorted(KEYS)
    assert float(g['max_rel_dev']) <= 2.855e-14 * (1 + 1e-3)
    for k in KEYS:
        nfev, acc, rej = (int(v) for v in g[k + '__counts'])
        nf = int(g[k + '__span'][2])
        if k.endswith('__rej'):
            assert rej > 0, k
        elif k.endswith('__max'):
            assert rej == 0 and acc <= nf + 1, k
        else:
            assert acc > nf + 1, k


@pytest.mark.parametrize('key', KEYS)
def test_restatement_takes_scipys_steps_and_ends_where_the_reference_does(key):
    g = golden('adaptive.npz')
    name, method, _ = key.split('__')
    t0, t1, nf = g[key + '__span']
    rtol, atol = g[key + '__tol']
    y, nfev, acc, rej, status = AR.solve(FIELDS[name](), method, t0, t1, int(nf), g[key + '__u0'], rtol=float(rtol),
                                         atol=float(atol))
    want = g[key + '__y']
    dev = float(np.max(np.abs(y - want) / np.abs(want)))
    print(f'{key}: nfev {nfev} accepted {acc} rejected {rej} deviation {dev:.3e}')
    assert status == 0
    assert (nfev, acc, rej) == tuple(int(v) for v in g[key + '__counts'])
    assert dev <= BOUND


def test_sum_order_is_columns_then_the_halving_tree():
    """hand-computed: big + 1.0 is big, so every order but the stated one gives another sum"""
    big = 1e16
    assert AR.tree_sum([1.0, 2.0]) == 3.0                               # d = 2: x0 + x1
    assert AR.tree_sum([big, 1.0, -big]) == 1.0                         # d = 3: (x0 + x2) + x1; in order: 0.0
    assert AR.tree_sum([big, 1.0, -big, 1.0]) == 2.0                    # d = 4: (x0 + x2) + (x1 + x3); in order: 1.0
    x = np.zeros(65)
    x[0], x[32], x[64] = big, -big, 1.0       # column 0 = big + 1.0 = big first, then + column 32: 0.0
    assert AR.tree_sum(x) == 0.0              # (a tree over the first 64, then + x[64], gives 1.0)
    x = np.zeros(130)
    x[0], x[64], x[128] = 1.0, big, -big      # column 0 = (1.0 + big) - big = 0.0
    x[1], x[65], x[129] = 3.0, 4.0, 5.0       # column 1 = 12.0
    assert AR.tree_sum(x) == 12.0             # the exact sum is 13.0
    assert AR.rms([3.0, 4.0]) == np.sqrt(25.0 / 2.0)
    # Python's min / max: a NaN second argument never wins, a NaN first argument stays
    assert AR.pymax(0.2, float('nan')) == 0.2 and np.isnan(AR.pymin(float('nan'), 1.0))
    assert AR.min_step_at(0.25) == 10 * 2.0**-54 and AR.min_step_at(0.0) == 10 * 5e-324


def test_restatement_ends_on_nan_and_on_the_cap():
    f = FIELDS['lorenz']()
    u0 = np.array([0.1, np.nan, 0.3])
    y, nfev, acc, rej, status = AR.solve(f, 'RK45', 0.25, 0.75, 4, u0)
    assert status == 1 and acc == 0 and 10 < rej < 60
    u0 = O.System('lorenz').fit([-15, -15, 20])
    full = AR.solve(f, 'RK45', 0.25, 0.75, 4, u0)
    assert full[4] == 0 and full[2] + full[3] > 3
    y, nfev, acc, rej, status = AR.solve(f, 'RK45', 0.25, 0.75, 4, u0, max_attempts=3)
    assert status == 2 and acc + rej == 3 and nfev == 2 + 3 * 6


# ------------------------------------------------------------------------------------------------
# Python surface
# ------------------------------------------------------------------------------------------------
def _field():
    import nngp_amd
    return nngp_amd, nngp_amd.Lorenz(normalization='-11').get_vector_field()


def test_method_names_follow_the_reference():
    nn, f = _field()
    for given, method in (('RK45', 'RK45'), ('RK4', 'RK45'), ('RK23', 'RK23'), ('RK2', 'RK23')):
        s = nn.SolverScipy(f, 6, 45, 'RK4', F=given)
        assert s.F == method and s.G == 'RK4' and (s.Ng, s.Nf) == (6, 45)
    s = nn.SolverScipy(f, 6, 45, 'RK1')
    assert s.F == 'RK45' and (s.rtol, s.atol, s.first_step, s.max_attempts) == (1e-3, 1e-6, None, 5500)
    assert isinstance(s, nn.SolverAbstr) and isinstance(s, nn.SolverRK) and not s.fma
    assert s.step_mode == nn._lib.STEP_FIXED and not s.coarse_is_paged() and s.last_stats is None
    import nngp_amd as again
    assert again.SolverScipy is nn.SolverScipy and 'SolverScipy' in nn.__all__


@pytest.mark.parametrize('name', ['DOP853', 'RK8', 'Radau', 'BDF', 'LSODA', 'RK1'])
def test_other_methods_are_refused_by_name(name):
    nn, f = _field()
    with pytest.raises(NotImplementedError, match='DOP853' if name == 'RK8' else name):
        nn.SolverScipy(f, 6, 45, 'RK4', F=name)


def test_unsupported_arguments_are_refused_by_name(monkeypatch):
    nn, f = _field()
    with pytest.raises(TypeError, match='atol'):
        nn.SolverScipy(f, 6, 45, 'RK4', atol=np.array([1e-6, 1e-6, 1e-6]))
    with pytest.raises(TypeError, match='rtol'):
        nn.SolverScipy(f, 6, 45, 'RK4', rtol=[1e-3, 1e-3, 1e-3])
    for kw in ('events', 'dense_output', 'vectorized', 'args', 't_eval', 'jac', 'thresh'):
        with pytest.raises(TypeError, match=kw):
            nn.SolverScipy(f, 6, 45, 'RK4', **{kw: None})
    for kw, v in (('rtol', 0.0), ('rtol', -1e-3), ('rtol', float('nan')), ('atol', -1e-6), ('atol', float('inf')),
                  ('first_step', 0.0), ('first_step', -0.1), ('max_attempts', 0), ('max_attempts', 2.5)):
        with pytest.raises(ValueError, match=kw):
            nn.SolverScipy(f, 6, 45, 'RK4', **{kw: v})
    with pytest.raises(NotImplementedError, match='fma'):
        nn.SolverScipy(f, 6, 45, 'RK4', fma=True)
    monkeypatch.setenv('NNGP_RK_CONTRACT', '1')
    with pytest.raises(NotImplementedError, match='NNGP_RK_CONTRACT'):
        nn.SolverScipy(f, 6, 45, 'RK4')


def test_small_rtol_is_raised_with_scipys_warning():
    nn, f = _field()
    with pytest.warns(UserWarning, match='rtol'):
        s = nn.SolverScipy(f, 6, 45, 'RK4', rtol=1e-15)
    assert s.rtol == 100 * np.finfo(float).eps
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert nn.SolverScipy(f, 6, 45, 'RK4', rtol=1e-13).rtol == 1e-13


def test_trajectories_and_the_legacy_driver_refuse_it():
    nn, f = _field()
    s = nn.SolverScipy(f, 6, 45, 'RK4')
    with pytest.raises(NotImplementedError):
        s.run_F_full(0.0, 0.5, np.zeros(3))
    with pytest.raises(NotImplementedError):
        s.run_F_traj_batch(None, None, None)
    u0 = f.ode.get_init_cond()
    for kw in (dict(F='RK45'), dict(F='RK23'), dict(F='RK4', solver=s)):
        args = dict(f=f, tspan=[0, 18], u0=u0, N=6, Ng=36, Nf=360, epsilon=5e-7, G='RK4')
        args.update(kw)
        with pytest.raises(NotImplementedError, match='SolverScipy'):
            nn.legacy.Parareal(**args)


# ------------------------------------------------------------------------------------------------
# C-ABI
# ------------------------------------------------------------------------------------------------
def test_argument_errors_are_reported_before_any_hip_call():
    import nngp_amd
    L = nngp_amd.lib()
    cs = nngp_amd._lib.CSystem(0, 3, 0, 0, (ctypes.c_double * 4)(), None)
    ref = ctypes.byref(cs)

    def call(sys=ref, method=45, n=1, nf=4, rtol=1e-3, atol=1e-6, first=0.0, cap=100):
        return L.nngp_rk_adaptive(sys, method, n, None, None, nf, rtol, atol, first, cap, None, None, None, None)

    nan, inf = float('nan'), float('inf')
    for kw, text in ((dict(sys=None), b'sys is NULL'), (dict(method=853), b'method'), (dict(method=4), b'method'),
                     (dict(nf=0), b'nf'), (dict(rtol=0.0), b'rtol'), (dict(rtol=-1.0), b'rtol'),
                     (dict(rtol=nan), b'rtol'), (dict(rtol=inf), b'rtol'), (dict(atol=-1e-9), b'atol'),
                     (dict(atol=nan), b'atol'), (dict(atol=inf), b'atol'), (dict(first=-0.1), b'first_step'),
                     (dict(first=nan), b'first_step'), (dict(cap=0), b'max_attempts'), (dict(n=-1), b'n_slices')):
        assert call(**kw) == -1, kw
        assert text in L.nngp_last_error(), (kw, L.nngp_last_error())
    # a polynomial system whose handle was never created, and one that was destroyed
    poly = nngp_amd._lib.CSystem(nngp_amd._lib.SYS_POLY, 2, 987654, 0, (ctypes.c_double * 4)(), None)
    assert call(sys=ctypes.byref(poly)) == -1 and b'handle' in L.nngp_last_error()
    ode = nngp_amd.PolyODE([[(1.0, (1,))], [(-1.0, (0,))]], [1.0, 0.0])
    poly = nngp_amd._lib.CSystem(nngp_amd._lib.SYS_POLY, 2, ode.nx, 0, (ctypes.c_double * 4)(), None)
    assert call(sys=ctypes.byref(poly), n=0) == 0
    ode.destroy()
    assert call(sys=ctypes.byref(poly), n=0) == -1 and b'handle' in L.nngp_last_error()
    assert call(n=0) == 0                      # an empty batch is a no-op
    assert call(atol=0.0, n=0) == 0            # atol = 0 is scipy's to allow
