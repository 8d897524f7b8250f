"""Every kernel form the Runge-Kutta host dispatch (csrc/nngp_rk.hip launch_lane / launch_field) can
choose, compared with the CPU oracle bit for bit at the edges of that dispatch:

  * the seven ODE systems on the lane-group kernel and on the one-lane-per-slice kernel, '-11' and
    identity, every tableau, both step modes, 1 / 2 / 3 / 8 steps (the group kernel's two-step loop
    with and without its remainder step) and slice counts around the group, wave and workgroup
    boundaries of both group widths (16 lanes per slice; ThomasLabyrinth 4);
  * the Burgers wave kernel at 1, 2, 3 and 4 elements per lane (d = 64 .. 256), where rows 0 and d-1
    associate their Laplacian differently and sit in the first / last register of lanes 0 / 63;
  * Burgers on the LDS field kernel in every layout pick_threads has (64 threads x 1 or 2, one
    element per thread in several waves, the 512-thread form of many slices, 256 threads x 5..8)
    and at sizes that are no multiple of anything, plus the single right-hand side;
  * the refusals at d < 3 and d > 2048;
  * nngp_rk_batch_grid (per-slice j0 on a global grid, exact end point) on the group, lane, wave,
    field and both point-pair kernels;
  * the contracted build of the same instantiations within its stated tolerance.

Floating-point results are compared as int64 bit patterns (np.array_equal cannot see the sign of
a zero); inputs hold no exact zero."""
import ctypes

import numpy as np
import pytest

import oracle as O
from diffreact_ref import DiffReactNP, rk_np
from systems_table import (ODE_SYSTEMS, burgers_h, burgers_u0, oracle_burgers, oracle_ode, product_burgers,
                           product_ode_norm)
from test_gpu_contract import TOL, _rel

pytestmark = pytest.mark.gpu

TABS = ['RK1', 'RK2', 'RK4', 'RK8']
MODES = ['fixed', 'linspace']
NORMS = pytest.mark.parametrize('norm', [True, False], ids=['norm11', 'identity'])


def _t(torch, a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device='cuda')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _mode(mode):
    return O.STEP_FIXED if mode == 'fixed' else O.STEP_LINSPACE


def _run(gpu, ode, tab, mode, steps, T0, T1, U0, fma=False):
    import torch
    s = gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=steps, F=tab, G='RK1', step_mode=mode, fma=fma)
    return s.run_F_batch(_t(torch, T0), _t(torch, T1), _t(torch, U0)).cpu().numpy()


def _oracle_each(so, tab, mode, steps, T0, T1, U0):
    return np.array([so.rk(int(tab[2:]), T0[i], T1[i], int(steps), U0[i], _mode(mode)) for i in range(len(U0))])


# ------------------------------------------------------------------------------------------------
# A1: ODE systems, group kernel == lane kernel == oracle
# ------------------------------------------------------------------------------------------------
ODE_STEPS = [1, 2, 3, 8]
# one group; a partial wave; one wave at 16 lanes per slice; across it; five groups past it; one
# wave at 4 lanes per slice; across it; a second workgroup at 4 lanes per slice
ODE_SLICES = [1, 3, 4, 5, 9, 16, 17, 65]


def _ode_states(name, norm, n, rng):
    """uniform in +-0.3 of the normalised box; identity: the same draws in the physical box"""
    U = rng.uniform(-0.3, 0.3, (n, len(O.BOUNDS[name][0])))
    if not norm:
        mn, mx = (np.asarray(b, dtype=float) for b in O.BOUNDS[name][:2])
        U = mn + (U + 1) / 2 * (mx - mn)
    assert not np.any(U == 0.0)
    return U


@pytest.mark.parametrize('tab', TABS)
@NORMS
@pytest.mark.parametrize('name', list(ODE_SYSTEMS))
def test_ode_group_and_lane_kernels_are_bitwise_the_oracle(gpu, monkeypatch, name, norm, tab):
    ode = product_ode_norm(gpu, name, norm)
    so = oracle_ode(name, norm)
    rng = np.random.default_rng(11)
    for mode in MODES:
        for steps in ODE_STEPS:
            for n in ODE_SLICES:
                U0 = _ode_states(name, norm, n, rng)
                T0 = rng.uniform(0, 1, n)
                T1 = T0 + 0.0025 * steps
                monkeypatch.setenv('NNGP_RK_GROUP', '1')
                grp = _run(gpu, ode, tab, mode, steps, T0, T1, U0)
                monkeypatch.setenv('NNGP_RK_GROUP', '0')
                lane = _run(gpu, ode, tab, mode, steps, T0, T1, U0)
                ora = _oracle_each(so, tab, mode, steps, T0, T1, U0)
                at = (mode, steps, n)
                assert np.all(np.isfinite(grp)) and np.all(np.isfinite(lane)) and np.all(np.isfinite(ora)), at
                assert np.array_equal(_bits(grp), _bits(lane)), at
                assert np.array_equal(_bits(grp), _bits(ora)), at
                assert np.array_equal(_bits(lane), _bits(ora)), at


# ------------------------------------------------------------------------------------------------
# Burgers: inputs shared by A2, A3, A5 and A6
# ------------------------------------------------------------------------------------------------
def _burgers_states(so, d, n, rng, rough=False):
    """The initial condition plus 1e-3 N(0,1), mapped through the normaliser of `so`; every second
    slice (1, 3, ..), or with `rough` every slice, is a uniform(-0.9, 0.9) draw instead.  Near the
    initial condition u[d-1], u[0] and u[1] are within 1e-3 of each other: row 0's three Laplacian
    terms cancel exactly in any order of summation, and a last-bit difference in row d-1 is mostly
    rounded away in u + h f.  On a rough state the three terms round differently in about two of
    five draws and h f is of the size of u, so a batch of ROUGH such slices tells the orders of both
    rows apart (h = burgers_h keeps the diffusion number at 0.1, the advective one below 0.09)."""
    U = np.ascontiguousarray(so.fit(burgers_u0(d)[None, :] + 1e-3 * rng.standard_normal((n, d))))
    if rough:
        U[:] = rng.uniform(-0.9, 0.9, U.shape)
    else:
        U[1::2] = rng.uniform(-0.9, 0.9, U[1::2].shape)
    assert not np.any(U == 0.0)
    return U


ROUGH = 64


def _burgers_spans(d, n, steps, nu=0.01):
    """each slice its own t0 and span; the longest is `steps` steps of the stable h"""
    T0 = 0.25 + 0.0625 * (np.arange(n) % 7)
    return T0, T0 + steps * burgers_h(d, nu) * (1 - 0.05 * (np.arange(n) % 5))


# ------------------------------------------------------------------------------------------------
# A2: the wave kernel, 1 to 4 elements per lane
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tab', TABS)
@NORMS
@pytest.mark.parametrize('d', [64, 128, 192, 256])
def test_burgers_wave_kernel_is_bitwise_the_oracle(gpu, monkeypatch, d, norm, tab):
    ode = product_burgers(gpu, d, norm)
    so = oracle_burgers(d, norm)
    rng = np.random.default_rng(d)
    for mode in MODES:
        for steps in (1, 2, 3):
            for n in (1, 5, ROUGH):
                U0 = _burgers_states(so, d, n, rng, rough=n == ROUGH)
                T0, T1 = _burgers_spans(d, n, steps)
                monkeypatch.delenv('NNGP_BURGERS_LDS', raising=False)
                wave = _run(gpu, ode, tab, mode, steps, T0, T1, U0)
                monkeypatch.setenv('NNGP_BURGERS_LDS', '1')
                lds = _run(gpu, ode, tab, mode, steps, T0, T1, U0)
                monkeypatch.delenv('NNGP_BURGERS_LDS')
                ora = _oracle_each(so, tab, mode, steps, T0, T1, U0)
                at = (mode, steps, n)
                assert np.all(np.isfinite(wave)) and np.all(np.isfinite(ora)), at
                assert np.array_equal(_bits(wave), _bits(ora)), at
                assert np.array_equal(_bits(wave), _bits(lds)), at


# ------------------------------------------------------------------------------------------------
# A3: Burgers on the LDS field kernel, every pick_threads branch
# ------------------------------------------------------------------------------------------------
# (d, slices): 64 threads x 1 (3, 4, 5, 63) and x 2 (65, 100, 127); one element per thread in 3, 5,
# 16 waves (129, 257 / 320, 1000 / 1024); 256 threads x 5 and x 8 (1025, 2048); and the 512-thread
# form once slices * ceil(d / 64) > 4096 (320: one element per thread; 1000: two)
FIELD_SIZES = [(d, 3) for d in (3, 4, 5, 63, 65, 100, 127, 129, 257, 320, 1000, 1024, 1025, 2048)] + \
              [(320, 820), (1000, 260)]


@pytest.mark.parametrize('tab', ['RK1', 'RK4', 'RK8'])
@pytest.mark.parametrize('d,n', FIELD_SIZES, ids=[f'{d}x{n}' for d, n in FIELD_SIZES])
def test_burgers_field_kernel_is_bitwise_the_oracle(gpu, monkeypatch, d, n, tab):
    monkeypatch.delenv('NNGP_RK_THREADS', raising=False)
    norm = d % 2 == 1           # '-11' on the odd sizes, identity on the even ones
    rng = np.random.default_rng(d + n)
    # the 3-slice cases once more with ROUGH rough slices (the same layout: pick_threads changes at
    # slices * ceil(d / 64) > 4096); half of the 820 / 260 slices are rough already.  Up to d = 5
    # also with nu = 1: at nu = 0.01 the step is the advective 0.1 dx, h nu / dx^2 < 3e-3, and the
    # Laplacian's last bit, hence the order of its terms, is rounded away in u + h f
    for nu in (0.01, 1.0) if d <= 5 else (0.01,):
        ode = product_burgers(gpu, d, norm, nu)
        so = oracle_burgers(d, norm, nu=nu)
        for m, rough in [(n, False)] + ([(ROUGH, True)] if n == 3 else []):
            U0 = _burgers_states(so, d, m, rng, rough)
            T0, T1 = _burgers_spans(d, m, 3, nu)
            for mode in MODES:
                got = _run(gpu, ode, tab, mode, 3, T0, T1, U0)
                ora = so.rk_batch(int(tab[2:]), T0, T1, 3, U0, _mode(mode))
                assert np.all(np.isfinite(got)) and np.all(np.isfinite(ora)), (nu, m, mode)
                assert np.array_equal(_bits(got), _bits(ora)), (nu, m, mode)


RHS_SIZES = [3, 4, 5, 63, 64, 65, 100, 127, 128, 129, 192, 256, 257, 320, 1000, 1024, 1025, 2048, 2049]


@NORMS
@pytest.mark.parametrize('d', RHS_SIZES)
def test_burgers_rhs_is_bitwise_the_oracle(gpu, d, norm):
    f = product_burgers(gpu, d, norm).get_vector_field()
    so = oracle_burgers(d, norm)
    rng = np.random.default_rng(2 * d + norm)
    U = np.vstack([_burgers_states(so, d, 2, rng), _burgers_states(so, d, ROUGH, rng, rough=True)])
    got = f(0.0, U)
    ora = np.array([so.rhs(u) for u in U])
    assert np.all(np.isfinite(got))
    assert np.array_equal(_bits(got), _bits(ora))


# ------------------------------------------------------------------------------------------------
# A4: refusals (host checks in field_args / launch_field, before any launch)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [2, 2049])
def test_burgers_propagator_refuses_sizes_outside_3_to_2048(gpu, d):
    import torch
    ode = gpu.Burgers(d_x=d)
    s = gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=3, F='RK4', G='RK1')
    U0 = _t(torch, np.tile(ode.get_init_cond(), (3, 1)) + 0.5)
    T0 = _t(torch, [0.0, 0.1, 0.2])
    with pytest.raises(gpu.NNGPError):
        s.run_F_batch(T0, T0 + 1e-3, U0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# A5: nngp_rk_batch_grid on every kernel form
# ------------------------------------------------------------------------------------------------
class _GridCase:
    """ode (product), ref(order, g0, g1, gsteps, j0, steps, u0) -> state, (g0, g1), states(n, rng)"""

    def __init__(self, ode, ref, span, states, group=None):
        self.ode, self.ref, self.span, self.states, self.group = ode, ref, span, states, group


PER, NGRID = 3, 4


# key -> (family, size or ODE name): the group kernel at 16 and at 4 lanes per slice and the lane
# kernel for both; the wave kernel at 1 and 3 elements per lane; the LDS field kernel (Burgers
# d = 65, FHN-PDE 4 x 4); the FHN-PDE and DiffReact point-pair kernels (16 x 16)
GRID_CASES = {
    'lorenz_group': ('ode', 'lorenz'), 'lorenz_lane': ('ode', 'lorenz'),
    'tomlab_group': ('ode', 'tomlab'), 'tomlab_lane': ('ode', 'tomlab'),
    'burgers64': ('burgers', 64), 'burgers192': ('burgers', 192), 'burgers65': ('burgers', 65),
    'fhnpde4': ('fhnpde', 4), 'fhnpde16': ('fhnpde', 16), 'diffreact16': ('diffreact', 16),
}


def _grid_case(gpu, key):
    gsteps = PER * NGRID
    family, what = GRID_CASES[key]
    if family == 'ode':
        name = what
        so = oracle_ode(name, True)
        return _GridCase(product_ode_norm(gpu, name, True), so.rk_grid, (0.125, 0.125 + 0.0025 * gsteps),
                         lambda n, rng: _ode_states(name, True, n, rng), group='0' if key.endswith('_lane') else '1')
    if family == 'burgers':
        d = what
        so = oracle_burgers(d, d != 192)
        return _GridCase(product_burgers(gpu, d, d != 192), so.rk_grid, (0.25, 0.25 + gsteps * burgers_h(d)),
                         lambda n, rng: _burgers_states(so, d, n, rng))
    nx = what
    if family == 'fhnpde':
        ode = gpu.FHN_PDE(d_x=nx)
        so = O.System('fhn_pde', nx=nx, normalized=False)
        u0 = ode.get_init_cond()
        return _GridCase(ode, so.rk_grid, (0.25, 0.3),
                         lambda n, rng: np.clip(u0[None, :] + 0.01 * rng.standard_normal((n, len(u0))), -1, 1))
    assert family == 'diffreact'
    f = DiffReactNP(nx)
    return _GridCase(gpu.DiffReact(d_x=nx),
                     lambda order, g0, g1, gs, j0, steps, u0: rk_np(f, order, g0, g1, steps, u0, 'linspace', gs, j0),
                     (0.25, 0.31), lambda n, rng: rng.uniform(-0.9, 0.9, (n, 2 * nx * nx)))


@pytest.mark.parametrize('tab', ['RK1', 'RK4'])
@pytest.mark.parametrize('key', list(GRID_CASES))
def test_rk_batch_grid_on_every_kernel_form(gpu, monkeypatch, key, tab):
    """4 slices of 3 steps on one grid of 12 (j0 = 3 i; the last slice ends on t[12] = g1 itself):
    chained one launch per slice, as the legacy initial coarse sweep does, and as one launch of four
    independent states with their own j0."""
    import torch
    from nngp_amd import _lib
    c = _grid_case(gpu, key)
    if c.group is not None:
        monkeypatch.setenv('NNGP_RK_GROUP', c.group)
    monkeypatch.delenv('NNGP_RK_THREADS', raising=False)
    monkeypatch.delenv('NNGP_BURGERS_LDS', raising=False)
    order = int(tab[2:])
    gsteps = PER * NGRID
    g0, g1 = c.span
    cs = c.ode.get_vector_field().csystem(torch.device('cuda'))
    L = gpu.lib()
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(5)
    S = c.states(NGRID, rng)
    assert not np.any(S == 0.0)
    d = S.shape[1]
    # chained
    U = torch.empty((NGRID + 1, d), dtype=torch.float64, device='cuda')
    U[0] = _t(torch, S[0])
    G0, G1 = _t(torch, [g0]), _t(torch, [g1])
    for i in range(NGRID):
        j0 = torch.tensor([i * PER], dtype=torch.int64, device='cuda')
        _lib.check(L.nngp_rk_batch_grid(ctypes.byref(cs), _lib.TABLEAU[tab], 1, G0.data_ptr(), G1.data_ptr(), gsteps,
                                        j0.data_ptr(), PER, U[i:i + 1].data_ptr(), U[i + 1:i + 2].data_ptr(), st))
    got = U.cpu().numpy()
    x = S[0]
    for i in range(NGRID):
        x = c.ref(order, g0, g1, gsteps, i * PER, PER, x)
        assert np.all(np.isfinite(x))
        assert np.array_equal(_bits(got[i + 1]), _bits(x)), i
    # one launch, each slice its own state, grid and j0
    G0b = g0 + 0.03125 * np.arange(NGRID)
    G1b = G0b + (g1 - g0)
    j0 = torch.tensor([i * PER for i in range(NGRID)], dtype=torch.int64, device='cuda')
    out = torch.empty((NGRID, d), dtype=torch.float64, device='cuda')
    Sd, G0d, G1d = _t(torch, S), _t(torch, G0b), _t(torch, G1b)
    _lib.check(L.nngp_rk_batch_grid(ctypes.byref(cs), _lib.TABLEAU[tab], NGRID, G0d.data_ptr(), G1d.data_ptr(), gsteps,
                                    j0.data_ptr(), PER, Sd.data_ptr(), out.data_ptr(), st))
    got = out.cpu().numpy()
    for i in range(NGRID):
        ref = c.ref(order, G0b[i], G1b[i], gsteps, i * PER, PER, S[i])
        assert np.all(np.isfinite(ref))
        assert np.array_equal(_bits(got[i]), _bits(ref)), i


# ------------------------------------------------------------------------------------------------
# A6: the contracted build of the same instantiations, within tests/test_gpu_contract.py's TOL
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tab', ['RK4', 'RK8'])
@NORMS
@pytest.mark.parametrize('d', [64, 192, 256])
def test_contracted_burgers_wave_within_tolerance_of_oracle(gpu, monkeypatch, d, norm, tab):
    monkeypatch.delenv('NNGP_BURGERS_LDS', raising=False)
    ode = product_burgers(gpu, d, norm)
    so = oracle_burgers(d, norm)
    U0 = _burgers_states(so, d, 5, np.random.default_rng(d))
    T0, T1 = _burgers_spans(d, 5, 8)
    for mode in MODES:
        out = _run(gpu, ode, tab, mode, 8, T0, T1, U0, fma=True)
        ora = _oracle_each(so, tab, mode, 8, T0, T1, U0)
        assert np.all(np.isfinite(out)), mode
        for i in range(5):
            assert _rel(out[i], ora[i]) <= TOL, (mode, i, _rel(out[i], ora[i]))


@pytest.mark.parametrize('tab', ['RK4', 'RK8'])
@pytest.mark.parametrize('group', ['1', '0'], ids=['group', 'lane'])
@pytest.mark.parametrize('name', ['tomlab', 'fhn_ode', 'rossler', 'brus', 'dblpend'])
def test_contracted_identity_odes_within_tolerance_of_oracle(gpu, monkeypatch, name, group, tab):
    monkeypatch.setenv('NNGP_RK_GROUP', group)
    ode = product_ode_norm(gpu, name, False)
    so = oracle_ode(name, False)
    rng = np.random.default_rng(13)
    U0 = _ode_states(name, False, 5, rng)
    T0 = rng.uniform(0, 1, 5)
    T1 = T0 + 0.0025 * 8
    for mode in MODES:
        out = _run(gpu, ode, tab, mode, 8, T0, T1, U0, fma=True)
        ora = _oracle_each(so, tab, mode, 8, T0, T1, U0)
        assert np.all(np.isfinite(out)), mode
        for i in range(5):
            assert _rel(out[i], ora[i]) <= TOL, (mode, i, _rel(out[i], ora[i]))
