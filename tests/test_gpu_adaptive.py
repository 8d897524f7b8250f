"""nngp_rk_adaptive / SolverScipy on the GPU against the restatement of the arithmetic contract
(tests/adaptive_ref.py, pinned to scipy on the CPU by tests/test_adaptive_host.py): end state, nfev,
accepted and rejected steps of every slice, bit for bit.

Every launch gives each slice its own start, length and state, so the lanes of a wave (lane form)
take different numbers of steps and reject independently, and one workgroup of a field launch ends
long before its neighbour; the tests assert from the restatement's own counts that this happens.
Three tolerance sets (rtol, atol, nf): 'max' nearly every step capped by max_step, 'rej' and 'clip'
sized by the controller, with rejected steps and a last step cut by t1.

Shapes.  Lane form: 1, 3 and 65 slices (one lane, a few, a full wave and one lane of a second
block).  Field form: d = 16 and 128 (Burgers), 32 (FHN-PDE), 18 (DiffReact), and a polynomial
field at d = 5, 65 (one element per thread: one wave, a partial second wave), 257 (two per
thread in 192 threads, the first d past the one-per-thread edge 256) and 1025 (four per thread in
320 threads, the first d past the two-per-thread edge 1024); 1 and 3 slices.

The restatement of a launch is computed once per (system, method, tolerance set) and shared."""
import ctypes

import numpy as np
import pytest

import adaptive_ref as AR
import oracle as O
from diffreact_ref import DiffReactNP
from poly_ref import D4_16, L96_BOUNDS, LORENZ, SMALL, PolyNP, lorenz96

pytestmark = pytest.mark.gpu

METHODS = ['RK23', 'RK45']
TOLS = {'max': (1e-3, 1e-6, 24), 'rej': (1e-6, 1e-9, 2), 'clip': (1e-5, 1e-8, 5)}   # rtol, atol, nf
N_LANE = 65

# name: (oracle name, parameters, normalised, product class, base slice length)
ODES = {
    'lorenz': ('lorenz', (), True, 'Lorenz', 0.3),
    'hopf': ('hopf', (500.0,), True, 'Hopf', 2.0),
    'tomlab': ('tomlab', (), True, 'ThomasLabyrinth', 0.3),
    'fhn_ode': ('fhn_ode', (), True, 'FHN_ODE', 2.0),
    'rossler': ('rossler', (), True, 'Rossler', 2.0),
    'brus': ('brus', (), True, 'Brusselator', 2.0),
    'dblpend': ('dblpend', (), True, 'DblPend', 1.0),
    'lorenz_id': ('lorenz', (), False, 'Lorenz', 0.3),
}
POLY_LANE = {'poly3': ('lorenz', LORENZ, 0.3), 'poly4': ('d4_16', D4_16, 1.0)}
LANE = list(ODES) + list(POLY_LANE)
FIELD = ['burgers16', 'burgers128', 'fhnpde4', 'diffreact3', 'l96_5', 'l96_65', 'l96_257', 'l96_1025']
FIELD_LEN = {'burgers16': 0.5, 'burgers128': 0.05, 'fhnpde4': 4.0, 'diffreact3': 4.0, 'l96_5': 0.4, 'l96_65': 0.4,
             'l96_257': 0.2, 'l96_1025': 0.1}


def _t(torch, a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device='cuda')


def ref_field(name):
    """the restated f(u) of a case"""
    if name in ODES:
        oname, param, norm, _, _ = ODES[name]
        return O.System(oname, normalized=norm, param=param).rhs
    if name in POLY_LANE:
        key, rows, _ = POLY_LANE[name]
        return PolyNP(rows, *SMALL[key][3])
    if name.startswith('burgers'):
        return O.System('burgers', d=int(name[7:]), param=(0.01,), mn=0, mx=1).rhs
    if name == 'fhnpde4':
        return O.System('fhn_pde', nx=4, normalized=False).rhs
    if name == 'diffreact3':
        return DiffReactNP(3)
    return PolyNP(lorenz96(int(name[4:])), *L96_BOUNDS)


def product_ode(gpu, name):
    if name in ODES:
        _, _, norm, cls, _ = ODES[name]
        return getattr(gpu, cls)(normalization='-11') if norm else getattr(gpu, cls)()
    if name in POLY_LANE:
        key, rows, _ = POLY_LANE[name]
        mn, mx = SMALL[key][3]
        return gpu.PolyODE(rows, SMALL[key][1], mn=mn, mx=mx, normalization='-11')
    if name.startswith('burgers'):
        return gpu.Burgers(d_x=int(name[7:]), normalization='-11')
    if name == 'fhnpde4':
        return gpu.FHN_PDE(d_x=4)
    if name == 'diffreact3':
        return gpu.DiffReact(d_x=3)
    d = int(name[4:])
    return gpu.PolyODE(lorenz96(d), np.full(d, 2.0), mn=L96_BOUNDS[0], mx=L96_BOUNDS[1], normalization='-11')


def base_state(name):
    """a state of the case's system, in the units its field takes (normalised where it is)"""
    if name in ODES:
        oname, param, norm, _, _ = ODES[name]
        u0 = np.array(O.BOUNDS[oname][2], dtype=float)
        return O.System(oname, normalized=norm, param=param).fit(u0)
    if name in POLY_LANE:
        key = POLY_LANE[name][0]
        mn, mx = (np.asarray(v, dtype=float) for v in SMALL[key][3])
        return 2 * (np.array(SMALL[key][1]) - mn) / (mx - mn) - 1
    if name.startswith('burgers'):
        d = int(name[7:])
        return 2 * (0.5 * (np.cos(4.5 * np.pi * np.linspace(-1, 1, num=d)) + 1)) - 1
    if name == 'fhnpde4':
        return np.random.default_rng(45).uniform(0.0, 1.0, 32)
    if name == 'diffreact3':
        return np.random.default_rng(46).uniform(-0.5, 0.5, 18)
    mn, mx = L96_BOUNDS
    d = int(name[4:])
    return 2 * ((2.0 + 3.0 * np.random.default_rng(d).uniform(-1, 1, d)) - mn) / (mx - mn) - 1


def launch_inputs(name, n):
    """n slices: each its own state, start and length (lane form: lengths 0.4 .. 1.6 of the base
    length in a scrambled order; field form: the second slice a tenth of its neighbours')"""
    base = base_state(name)
    rng = np.random.default_rng(1000 + len(name) + n)
    U0 = base[None, :] + 0.02 * rng.uniform(-1, 1, (n, base.size))
    assert not np.any(U0 == 0.0)
    T0 = 0.25 + 0.0625 * np.arange(n)
    if name in FIELD:
        T1 = T0 + FIELD_LEN[name] * np.array([1.0, 0.1, 1.7])[:n]
    else:
        length = ODES[name][4] if name in ODES else POLY_LANE[name][2]
        T1 = T0 + length * (0.4 + 1.2 * ((7 * np.arange(n)) % N_LANE) / (N_LANE - 1))
    return U0, T0, T1


_REF = {}


def reference(name, method, tol, n, **kw):
    """the restatement of the n-slice launch of a case: (end states, stats [n][4])"""
    key = (name, method, tol, n, tuple(sorted(kw.items())))
    if key not in _REF:
        U0, T0, T1 = launch_inputs(name, n)
        rtol, atol, nf = TOLS[tol]
        _REF[key] = AR.solve_batch(ref_field(name), method, T0, T1, nf, U0, rtol=rtol, atol=atol, **kw)
    return _REF[key]


_ODE = {}


def _ode(gpu, name):
    if name not in _ODE:
        _ODE[name] = product_ode(gpu, name)
    return _ODE[name]


def run(gpu, name, method, tol, U0, T0, T1, out=None, stream=None, first_step=0.0, max_attempts=None):
    """one nngp_rk_adaptive launch: (end states, stats) as numpy"""
    import torch
    from nngp_amd import _lib
    rtol, atol, nf = TOLS[tol]
    u0 = U0 if torch.is_tensor(U0) else _t(torch, U0)
    n = u0.shape[0]
    uF = torch.empty_like(u0) if out is None else out
    stats = torch.full((max(n, 1), 4), -7, dtype=torch.int64, device='cuda')
    cs = _ode(gpu, name).get_vector_field().csystem(u0.device)
    t0, t1 = _t(torch, T0), _t(torch, T1)
    st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    cap = 100 * nf + 1000 if max_attempts is None else max_attempts
    _lib.check(_lib.lib().nngp_rk_adaptive(ctypes.byref(cs), AR.METHOD_CODE[method], n, t0.data_ptr(), t1.data_ptr(), nf,
                                           rtol, atol, first_step, cap, u0.data_ptr(), uF.data_ptr(), stats.data_ptr(),
                                           st))
    torch.cuda.synchronize()
    return uF.cpu().numpy(), stats.cpu().numpy()[:n]


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ------------------------------------------------------------------------------------------------
# lane form
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', LANE)
@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('tol', list(TOLS))
def test_lane_form_is_bitwise_the_restatement(gpu, name, method, tol):
    want = reference(name, method, tol, N_LANE)
    st = want[1]
    print(f'{name} {method} {tol}: accepted {st[:, 2].min()}..{st[:, 2].max()}, rejected {st[:, 3].sum()}')
    assert np.all(st[:, 0] == 0) and np.all(np.isfinite(want[0]))
    if tol != 'max':
        assert len(set(st[:, 2])) > 1              # the lanes of the wave take different step counts
    if tol == 'rej':
        assert st[:, 3].sum() > 0 and len(set(st[:, 3])) > 1    # and reject independently
    U0, T0, T1 = launch_inputs(name, N_LANE)
    got = run(gpu, name, method, tol, U0, T0, T1)
    assert same(got, want)
    # 3 slices and single slices: the same rows, bit for bit
    assert same(run(gpu, name, method, tol, U0[:3], T0[:3], T1[:3]), (want[0][:3], want[1][:3]))
    for i in (0, 37, 64):
        assert same(run(gpu, name, method, tol, U0[i:i + 1], T0[i:i + 1], T1[i:i + 1]),
                    (want[0][i:i + 1], want[1][i:i + 1])), i


# ------------------------------------------------------------------------------------------------
# field form
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FIELD)
@pytest.mark.parametrize('method', METHODS)
def test_field_form_is_bitwise_the_restatement(gpu, name, method):
    for tol in TOLS:
        want = reference(name, method, tol, 3)
        st = want[1]
        print(f'{name} {method} {tol}: accepted {st[:, 2]}, rejected {st[:, 3]}')
        assert np.all(st[:, 0] == 0) and np.all(np.isfinite(want[0]))
        if tol == 'rej':
            assert 2 * st[1, 2] <= st[2, 2]         # the middle slice ends long before its neighbour
        U0, T0, T1 = launch_inputs(name, 3)
        assert same(run(gpu, name, method, tol, U0, T0, T1), want), tol
        assert same(run(gpu, name, method, tol, U0[2:], T0[2:], T1[2:]), (want[0][2:], want[1][2:])), tol
    # at least one case of the system rejects a step
    assert sum(reference(name, m, tol, 3)[1][:, 3].sum() for m in METHODS for tol in TOLS) > 0


# ------------------------------------------------------------------------------------------------
# statuses
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['lorenz', 'poly4', 'burgers16', 'l96_257'])
@pytest.mark.parametrize('method', METHODS)
def test_nan_state_ends_with_status_1_and_the_cap_with_status_2(gpu, name, method):
    import torch
    U0, T0, T1 = launch_inputs(name, 3)
    U0[1, U0.shape[1] // 2] = np.nan
    f = ref_field(name)
    rtol, atol, nf = TOLS['rej']
    want = AR.solve_batch(f, method, T0, T1, nf, U0, rtol=rtol, atol=atol)
    assert list(want[1][:, 0]) == [0, 1, 0] and want[1][1, 2] == 0 and 10 < want[1][1, 3] < 100
    got = run(gpu, name, method, 'rej', U0, T0, T1)
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0], want[0], equal_nan=True)      # the NaN slice keeps its initial state
    # the cap: three attempted steps of a slice that needs more
    U0, T0, T1 = launch_inputs(name, 3)
    want = AR.solve_batch(f, method, T0, T1, nf, U0, rtol=rtol, atol=atol, max_attempts=3)
    assert want[1][2, 0] == 2 and want[1][2, 2] + want[1][2, 3] == 3 and want[1][2, 2] > 0
    assert same(run(gpu, name, method, 'rej', U0, T0, T1, max_attempts=3), want)
    # the Python surface raises for both, naming the slice
    s = gpu.SolverScipy(_ode(gpu, name).get_vector_field(), 1, nf, 'RK1', F=method, rtol=rtol, atol=atol, max_attempts=3)
    with pytest.raises(gpu.NNGPError, match='max_attempts'):
        s.run_F_batch(_t(torch, T0), _t(torch, T1), _t(torch, U0))
    assert s.last_stats['status'][2] == 2
    s = gpu.SolverScipy(_ode(gpu, name).get_vector_field(), 1, nf, 'RK1', F=method, rtol=rtol, atol=atol)
    U0[1, 0] = np.nan
    with pytest.raises(gpu.NNGPError, match='slice 1 of 3.*min_step'):
        s.run_F_batch(_t(torch, T0), _t(torch, T1), _t(torch, U0))
    assert list(s.last_stats['status']) == [0, 1, 0]


# ------------------------------------------------------------------------------------------------
# the rest of the entry point
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['brus', 'fhnpde4'])
def test_first_step_aliasing_side_stream_and_empty_batch(gpu, name):
    import torch
    n = 3
    U0, T0, T1 = launch_inputs(name, n)
    rtol, atol, nf = TOLS['clip']
    h1 = float(np.min(T1 - T0)) / 7
    want = AR.solve_batch(ref_field(name), 'RK45', T0, T1, nf, U0, rtol=rtol, atol=atol, first_step=h1)
    assert np.all(want[1][:, 1] == 1 + 6 * (want[1][:, 2] + want[1][:, 3]))     # no evaluation for the first step
    assert same(run(gpu, name, 'RK45', 'clip', U0, T0, T1, first_step=h1), want)
    plain = reference(name, 'RK45', 'clip', n)
    u = _t(torch, U0)
    assert same(run(gpu, name, 'RK45', 'clip', u, T0, T1, out=u), plain)        # uF aliases u0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    assert same(run(gpu, name, 'RK45', 'clip', U0, T0, T1, stream=side.cuda_stream), plain)
    empty = run(gpu, name, 'RK45', 'clip', torch.empty((0, U0.shape[1]), dtype=torch.float64, device='cuda'),
                np.zeros(0), np.zeros(0))
    assert empty[0].shape == (0, U0.shape[1])
    # the Python surface: the same rows, the stats, a side stream, the single-slice forms
    s = gpu.SolverScipy(_ode(gpu, name).get_vector_field(), 1, nf, 'RK1', F='RK4', rtol=rtol, atol=atol)
    out = s.run_F_batch(_t(torch, T0), _t(torch, T1), _t(torch, U0), stream=side.cuda_stream)
    assert np.array_equal(out.cpu().numpy(), plain[0])
    for col, key in ((0, 'status'), (1, 'nfev'), (2, 'n_accepted'), (3, 'n_rejected')):
        assert np.array_equal(s.last_stats[key], plain[1][:, col])
    assert np.array_equal(s.run_F(T0[1], T1[1], U0[1]), plain[0][1])
    y, secs = s.run_F_timed(T0[2], T1[2], U0[2])
    assert np.array_equal(y, plain[0][2]) and secs > 0 and s.last_stats['nfev'][0] == plain[1][2, 1]
    s = gpu.SolverScipy(_ode(gpu, name).get_vector_field(), 1, nf, 'RK1', rtol=rtol, atol=atol, first_step=h1)
    assert np.array_equal(s.run_F_batch(T0, T1, _t(torch, U0)).cpu().numpy(), want[0])
    with pytest.raises(ValueError, match='first_step'):
        gpu.SolverScipy(_ode(gpu, name).get_vector_field(), 1, nf, 'RK1', first_step=10.0).run_F_batch(T0, T1, _t(torch, U0))
    assert s.run_F_batch(T0[:0], T1[:0], _t(torch, U0[:0])).shape == (0, U0.shape[1])
    with pytest.raises(NotImplementedError):
        gpu.Parareal(_ode(gpu, name), s, [0, 4], 4, verbose=None).build_cont_traj(
            dict(t=np.linspace(0, 4, 5), u=np.zeros((5, U0.shape[1]))))


# ------------------------------------------------------------------------------------------------
# driver
# ------------------------------------------------------------------------------------------------
def test_parareal_with_the_adaptive_fine_solver(gpu):
    """classic Parareal with an epsilon no slice meets: K = N, and boundary i is the fine solver
    applied i times (the driver copies the first unconverged slice's fine state forward).  The
    returned history ends with iterate K - 1, as the reference's (u[:, :, :k + 1]), in which the
    boundaries 0 .. N - 1 are the serial fine solution and boundary N is still the corrected one."""
    N, nf, rtol, atol = 4, 10, 1e-6, 1e-9
    ode = gpu.FHN_ODE(normalization='-11')
    s = gpu.SolverScipy(ode.get_vector_field(), 4, nf, 'RK2', F='RK45', rtol=rtol, atol=atol)
    r = gpu.Parareal(ode, s, [0, 8], N, epsilon=1e-300, verbose=None).run(model='parareal')
    assert r['k'] == N
    f = ref_field('fhn_ode')
    t = np.linspace(0, 8, N + 1)
    u, rejected = ode.get_init_cond(), 0
    for i in range(N):
        assert np.array_equal(r['u'][i, :, -1], u), i
        u, _, _, rej, status = AR.solve(f, 'RK45', t[i], t[i + 1], nf, u, rtol=rtol, atol=atol)
        rejected += rej
        assert status == 0
    assert rejected > 0 and np.all(np.isfinite(r['u'][N, :, -1]))
    assert s.last_stats['status'].shape == (1,)        # the last sweep integrated the last slice alone
    for model in ('nngp', 'elm'):
        r = gpu.Parareal(ode, s, [0, 8], 8, epsilon=5e-7, verbose=None).run(model=model, nn=5, seed=45)
        assert r['converged'] and r['k'] <= 8
        assert s.last_stats['nfev'].size >= 1 and np.all(s.last_stats['status'] == 0)
        assert np.all(s.last_stats['n_accepted'] > 0)
    r = gpu.PararealLight(ode, s, [0, 8], 8, epsilon=5e-7, verbose=None).run(model='gpjax')
    assert r['converged'] and r['k'] <= 8
