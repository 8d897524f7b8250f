"""The sampled-trajectory launch (nngp_rk_traj -> SolverRK.run_F_traj_batch / run_F_full ->
Parareal.build_cont_traj) on every kernel form of the Runge-Kutta host dispatch, bit for bit against
a prefix oracle: row p of a slice is the state after min(p * every, steps) steps, so it equals

  * LINSPACE: so.rk_grid(order, t0, t1, steps, 0, q, u0), the first q steps of the slice's grid;
  * FIXED:    q chained single steps so.rk(order, 0.0, h, 1, u) with h = (t1 - t0) / steps in float64
              ((h - 0.0) / 1 is exactly h; every right-hand side here ignores t, Hopf carries time in
              its state);
  * DiffReact: the same two with diffreact_ref.rk_np.

The (steps, every) pairs put samples on the first step of the group kernel's two-step loop, on its
second step and on its remainder step, and include every > steps (only u0 and the end).  Exact
builds are compared as int64 bit patterns; the contracted build within test_gpu_contract's TOL."""
import ctypes

import numpy as np
import pytest

import oracle as O
from diffreact_ref import DiffReactNP, rk_np
from systems_table import (ODE_SYSTEMS, burgers_h, burgers_u0, oracle_burgers, oracle_ode, product_burgers,
                           product_ode_norm)
from test_gpu_contract import TOL, _rel

pytestmark = pytest.mark.gpu

MODES = ['fixed', 'linspace']
STEPS_EVERY = [(1, 1), (2, 1), (3, 1), (8, 1), (8, 3), (7, 2), (5, 4), (3, 5)]


def _t(torch, a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device='cuda')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _rows(steps, every):
    return 1 + -(-steps // every)


class _Case:
    """One kernel form: the product ODE, the two single-slice references
         lin(order, t0, t1, steps, q, u0) -> state after the first q steps of the slice's grid
         fix(order, h, u)                 -> state after one step of size h
    its input states and per-slice spans, and the environment that selects the form."""

    def __init__(self, ode, lin, fix, states, spans, env):
        self.ode, self.lin, self.fix, self.states, self.spans, self.env = ode, lin, fix, states, spans, env

    def setenv(self, monkeypatch):
        for k in ('NNGP_RK_GROUP', 'NNGP_RK_THREADS', 'NNGP_BURGERS_LDS', 'NNGP_FHN_PAIR'):
            monkeypatch.delenv(k, raising=False)
        for k, v in self.env.items():
            monkeypatch.setenv(k, v)

    def prefix(self, order, mode, t0, t1, steps, every, u0):
        """the [n_out][d] rows of one slice"""
        rows = [np.array(u0, dtype=np.float64)]
        if mode == 'linspace':
            for p in range(1, _rows(steps, every)):
                rows.append(self.lin(order, t0, t1, steps, min(p * every, steps), u0))
        else:
            h = (np.float64(t1) - np.float64(t0)) / np.float64(steps)
            u, q = rows[0], 0
            for p in range(1, _rows(steps, every)):
                while q < min(p * every, steps):
                    u = self.fix(order, h, u)
                    q += 1
                rows.append(u)
        return np.array(rows)


def _system_case(ode, so, states, spans, env):
    return _Case(ode, lambda order, t0, t1, steps, q, u0: so.rk_grid(order, t0, t1, steps, 0, q, u0),
                 lambda order, h, u: so.rk(order, 0.0, h, 1, u), states, spans, env)


def _ode_states(name, norm, n, rng):
    """uniform in +-0.3 of the normalised box; identity: the same draws in the physical box"""
    U = rng.uniform(-0.3, 0.3, (n, len(O.BOUNDS[name][0])))
    if not norm:
        mn, mx = (np.asarray(b, dtype=float) for b in O.BOUNDS[name][:2])
        U = mn + (U + 1) / 2 * (mx - mn)
    assert not np.any(U == 0.0)
    return U


def _ode_case(gpu, name, norm, group):
    def spans(n, steps, rng):
        T0 = rng.uniform(0, 1, n)
        return T0, T0 + 0.0025 * steps
    return _system_case(product_ode_norm(gpu, name, norm), oracle_ode(name, norm),
                        lambda n, rng: _ode_states(name, norm, n, rng), spans, {'NNGP_RK_GROUP': group})


def _burgers_case(gpu, d, norm):
    so = oracle_burgers(d, norm)

    def states(n, rng):
        # the initial condition plus noise, and every second slice a rough uniform draw: there the
        # Laplacian's terms of rows 0 and d-1 round differently in another order of summation
        U = np.ascontiguousarray(so.fit(burgers_u0(d)[None, :] + 1e-3 * rng.standard_normal((n, d))))
        U[1::2] = rng.uniform(-0.9, 0.9, U[1::2].shape)
        assert not np.any(U == 0.0)
        return U

    def spans(n, steps, rng):
        T0 = 0.25 + 0.0625 * (np.arange(n) % 7)
        return T0, T0 + steps * burgers_h(d) * (1 - 0.05 * (np.arange(n) % 5))
    return _system_case(product_burgers(gpu, d, norm), so, states, spans, {})


def _pde_spans(h):
    def spans(n, steps, rng):
        T0 = 0.25 + 0.03125 * np.arange(n)
        return T0, T0 + steps * h * (1 - 0.05 * (np.arange(n) % 5))
    return spans


def _fhnpde_case(gpu, nx):
    ode = gpu.FHN_PDE(d_x=nx)
    so = O.System('fhn_pde', nx=nx, normalized=False)
    u0 = ode.get_init_cond()
    return _system_case(ode, so, lambda n, rng: np.clip(u0[None, :] + 0.01 * rng.standard_normal((n, len(u0))), -1, 1),
                        _pde_spans(0.004), {})


def _diffreact_case(gpu, nx):
    f = DiffReactNP(nx)
    return _Case(gpu.DiffReact(d_x=nx),
                 lambda order, t0, t1, steps, q, u0: rk_np(f, order, t0, t1, q, u0, 'linspace', steps, 0),
                 lambda order, h, u: rk_np(f, order, 0.0, h, 1, u, 'fixed'),
                 lambda n, rng: rng.uniform(-0.9, 0.9, (n, 2 * nx * nx)), _pde_spans(0.005), {})


# key -> (builder(gpu, norm), tableaux, normalisations, slice counts): the group kernel at 16 lanes per
# slice (Lorenz, Hopf with its carried registers) and at 4 (Thomas labyrinth), the lane kernel for both
# widths, the Burgers wave kernel at 1 and 3 elements per lane, the LDS field kernel at 64 threads x 2
# (Burgers 65), 256 threads x 5 (1025, the 8-element form) and FHN-PDE 4 x 4, and the FHN-PDE and
# DiffReact point-pair kernels (16 x 16).  17 slices cross a workgroup at both group widths.
ODE_N, FIELD_N = (1, 5, 17), (1, 3)
BOTH, IDENT = (True, False), (False,)
FORMS = {
    'lorenz_group': (lambda g, nm: _ode_case(g, 'lorenz', nm, '1'), ('RK1', 'RK4'), BOTH, ODE_N),
    'hopf_group': (lambda g, nm: _ode_case(g, 'hopf', nm, '1'), ('RK1', 'RK4', 'RK8'), BOTH, ODE_N),
    'tomlab_group': (lambda g, nm: _ode_case(g, 'tomlab', nm, '1'), ('RK1', 'RK4'), BOTH, ODE_N),
    'lorenz_lane': (lambda g, nm: _ode_case(g, 'lorenz', nm, '0'), ('RK1', 'RK4'), BOTH, ODE_N),
    'tomlab_lane': (lambda g, nm: _ode_case(g, 'tomlab', nm, '0'), ('RK1', 'RK4'), BOTH, ODE_N),
    'burgers64': (lambda g, nm: _burgers_case(g, 64, nm), ('RK1', 'RK4', 'RK8'), BOTH, FIELD_N),
    'burgers192': (lambda g, nm: _burgers_case(g, 192, nm), ('RK1', 'RK4'), BOTH, FIELD_N),
    'burgers65': (lambda g, nm: _burgers_case(g, 65, nm), ('RK1', 'RK4'), BOTH, FIELD_N),
    'burgers1025': (lambda g, nm: _burgers_case(g, 1025, nm), ('RK1', 'RK4'), BOTH, FIELD_N),
    'fhnpde4': (lambda g, nm: _fhnpde_case(g, 4), ('RK1', 'RK4'), IDENT, FIELD_N),
    'fhnpde16': (lambda g, nm: _fhnpde_case(g, 16), ('RK1', 'RK4', 'RK8'), IDENT, FIELD_N),
    'diffreact16': (lambda g, nm: _diffreact_case(g, 16), ('RK1', 'RK4'), IDENT, FIELD_N),
}
FORM_PARAMS = [pytest.param(key, tab, norm, id=f"{key}-{tab}-{'norm11' if norm else 'identity'}")
               for key, (_, tabs, norms, _) in FORMS.items() for tab in tabs for norm in norms]


def _check_case(gpu, c, tab, mode, steps, every, n, rng, fma=False):
    """one trajectory launch of n slices against the prefix oracle; returns the worst relative
    difference (the exact build must have none)"""
    import torch
    order = int(tab[2:])
    s = gpu.SolverRK(c.ode.get_vector_field(), Ng=steps, Nf=steps, F=tab, G=tab, step_mode=mode, fma=fma)
    U0 = c.states(n, rng)
    T0, T1 = c.spans(n, steps, rng)
    U0d, T0d, T1d = _t(torch, U0), _t(torch, T0), _t(torch, T1)
    traj = s.run_F_traj_batch(T0d, T1d, U0d, every=every)
    assert tuple(traj.shape) == (n, _rows(steps, every), U0.shape[1]) == (n, s.traj_rows(steps, every), U0.shape[1])
    got = traj.cpu().numpy()
    end = s.run_F_batch(T0d, T1d, U0d).cpu().numpy()
    same = s.run_G_traj_batch(T0d, T1d, U0d, every=every).cpu().numpy()
    at = (mode, steps, every, n)
    assert np.all(np.isfinite(got)), at
    assert np.array_equal(_bits(got[:, 0]), _bits(U0)), at
    assert np.array_equal(_bits(got[:, -1]), _bits(end)), at     # the end state the run itself uses
    assert np.array_equal(_bits(got), _bits(same)), at           # G of the same tableau and step count
    worst = 0.0
    for i in range(n):
        ref = c.prefix(order, mode, T0[i], T1[i], steps, every, U0[i])
        assert np.all(np.isfinite(ref)), at
        if fma:
            worst = max(worst, max(_rel(got[i, p], ref[p]) for p in range(len(ref))))
        else:
            assert np.array_equal(_bits(got[i]), _bits(ref)), at + (i,)
    return worst


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('key,tab,norm', FORM_PARAMS)
def test_trajectory_rows_are_bitwise_the_prefix_oracle(gpu, monkeypatch, key, tab, norm, mode):
    build, _, _, slices = FORMS[key]
    c = build(gpu, norm)
    c.setenv(monkeypatch)
    rng = np.random.default_rng(17)
    for steps, every in STEPS_EVERY:
        for n in slices:
            _check_case(gpu, c, tab, mode, steps, every, n, rng)


@pytest.mark.parametrize('norm', BOTH, ids=['norm11', 'identity'])
@pytest.mark.parametrize('name', [k for k in ODE_SYSTEMS if k not in ('lorenz', 'hopf')])
def test_every_group_specialisation_samples_bitwise(gpu, monkeypatch, name, norm):
    """the other five ODE systems on the group kernel (each its own GroupSys)"""
    c = _ode_case(gpu, name, norm, '1')
    c.setenv(monkeypatch)
    rng = np.random.default_rng(19)
    for mode in MODES:
        _check_case(gpu, c, 'RK4', mode, 7, 2, 5, rng)


@pytest.mark.parametrize('tab', ['RK4', 'RK8'])
@pytest.mark.parametrize('key', ['hopf_group', 'burgers64', 'fhnpde16'])
def test_contracted_trajectory_within_tolerance_of_prefix_oracle(gpu, monkeypatch, key, tab):
    build, _, norms, slices = FORMS[key]
    c = build(gpu, norms[0])
    c.setenv(monkeypatch)
    rng = np.random.default_rng(23)
    for mode in MODES:
        worst = _check_case(gpu, c, tab, mode, 8, 3, slices[-1], rng, fma=True)
        assert worst <= TOL, (mode, worst)


def test_empty_batch_returns_an_empty_trajectory(gpu):
    import torch
    s = gpu.SolverRK(gpu.Lorenz(normalization='-11').get_vector_field(), Ng=6, Nf=8, F='RK4', G='RK4')
    e = torch.empty((0,), dtype=torch.float64, device='cuda')
    out = s.run_F_traj_batch(e, e, torch.empty((0, 3), dtype=torch.float64, device='cuda'), every=3)
    assert tuple(out.shape) == (0, 4, 3)


def test_trajectory_launch_keeps_the_propagator_refusals(gpu):
    import torch
    ode = gpu.Burgers(d_x=2049)
    s = gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=3, F='RK4', G='RK1')
    U0 = _t(torch, np.tile(ode.get_init_cond(), (3, 1)) + 0.5)
    T0 = _t(torch, [0.0, 0.1, 0.2])
    with pytest.raises(gpu.NNGPError):
        s.run_F_traj_batch(T0, T0 + 1e-3, U0)
    torch.cuda.synchronize()


def test_row_offsets_are_64_bit(gpu, monkeypatch):
    """n_slices * n_out * d past 2^31 doubles: the last slices' blocks start beyond a 32-bit element
    offset.  Burgers d = 2048, RK1, 1000 stable steps at every = 1; the last slice's block equals the
    same slice launched alone (whose rows the tests above pin to the oracle)."""
    import torch
    for k in ('NNGP_RK_THREADS', 'NNGP_BURGERS_LDS'):
        monkeypatch.delenv(k, raising=False)
    d, n, steps = 2048, 1050, 1000
    assert n * (steps + 1) * d > 2**31 and (n - 1) * (steps + 1) * d > 2**31
    free, _ = torch.cuda.mem_get_info()
    if free < 20 * 2**30:
        pytest.skip('needs 17 GiB of device memory for the trajectory')
    ode = gpu.Burgers(d_x=d)
    s = gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=steps, F='RK1', G='RK1')
    rng = np.random.default_rng(29)
    U0 = _t(torch, burgers_u0(d)[None, :] + 1e-3 * rng.standard_normal((n, d)))
    T0 = _t(torch, 0.25 + 1e-3 * np.arange(n))
    T1 = T0 + steps * burgers_h(d)
    traj = s.run_F_traj_batch(T0, T1, U0)
    assert tuple(traj.shape) == (n, steps + 1, d)
    for i in (0, n - 1):
        alone = s.run_F_traj_batch(T0[i:i + 1], T1[i:i + 1], U0[i:i + 1])
        assert torch.equal(traj[i].view(torch.int64), alone[0].view(torch.int64)), i
        assert bool(torch.isfinite(alone).all())
    del traj
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# run_F_full / run_G_full: numpy in and out, RK.run's np.linspace grid
# ------------------------------------------------------------------------------------------------
def _one_launch_per_point(gpu, ode, tab, t0, t1, steps, u0):
    """what run_F_full computed before the trajectory launch: one single-step FIXED nngp_rk_batch
    launch per np.linspace point"""
    import torch
    from nngp_amd import _lib
    cs = ode.get_vector_field().csystem(torch.device('cuda'))
    st = torch.cuda.current_stream().cuda_stream
    t = np.linspace(t0, t1, num=steps + 1)
    out = np.empty((steps + 1, len(u0)))
    out[0] = u0
    cur = _t(torch, np.asarray(u0, dtype=np.float64).reshape(1, -1))
    nxt = torch.empty_like(cur)
    for n in range(steps):
        ta, tb = _t(torch, [t[n]]), _t(torch, [t[n + 1]])
        _lib.check(_lib.lib().nngp_rk_batch(ctypes.byref(cs), _lib.TABLEAU[tab], _lib.STEP_FIXED, 1, ta.data_ptr(),
                                             tb.data_ptr(), 1, cur.data_ptr(), nxt.data_ptr(), st))
        cur, nxt = nxt, cur
        out[n + 1] = cur[0].cpu().numpy()
    return out


@pytest.mark.parametrize('key', ['lorenz_group', 'burgers65'])
def test_run_full_is_what_it_was_and_the_linspace_prefix_oracle(gpu, monkeypatch, key):
    c = FORMS[key][0](gpu, True)
    c.setenv(monkeypatch)
    steps, tab = 8, 'RK4'
    rng = np.random.default_rng(31)
    u0 = c.states(1, rng)[0]
    T0, T1 = c.spans(1, steps, rng)
    t0, t1 = float(T0[0]), float(T1[0])
    s = gpu.SolverRK(c.ode.get_vector_field(), Ng=steps, Nf=steps, F=tab, G=tab)   # FIXED: full is LINSPACE anyway
    full = s.run_F_full(t0, t1, u0)
    assert full.shape == (steps + 1, len(u0)) and np.all(np.isfinite(full))
    assert np.array_equal(_bits(full[0]), _bits(u0))
    assert np.array_equal(_bits(full), _bits(_one_launch_per_point(gpu, c.ode, tab, t0, t1, steps, u0)))
    assert np.array_equal(_bits(full), _bits(c.prefix(4, 'linspace', t0, t1, steps, 1, u0)))
    assert np.array_equal(_bits(s.run_G_full(t0, t1, u0)), _bits(full))
    sparse = s.run_F_full(t0, t1, u0, every=3)
    assert np.array_equal(_bits(sparse), _bits(full[[0, 3, 6, 8]]))


# ------------------------------------------------------------------------------------------------
# Parareal.build_cont_traj
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lorenz_run(gpu):
    ode = gpu.Lorenz(normalization='-11')
    solver = gpu.SolverRK(ode.get_vector_field(), Ng=6, Nf=45, F='RK4', G='RK4')
    p = gpu.Parareal(ode, solver, [0, 4], 8, verbose=None)
    r = p.run(model='parareal', early_stop=2)
    return ode, solver, p, r, p.build_cont_traj()


def test_build_cont_traj_blocks_are_the_fine_trajectories(gpu, lorenz_run):
    ode, solver, p, r, dense = lorenz_run
    so = oracle_ode('lorenz', True)
    N, Nf = 8, 45
    assert dense.shape == (N * (Nf + 1), 3) and np.all(np.isfinite(dense))
    t = r['t']
    for i in range(N):
        blk = dense[i * (Nf + 1):(i + 1) * (Nf + 1)]
        u0 = r['u'][i, :, -1]
        assert np.array_equal(_bits(blk[0]), _bits(u0)), i
        ref = np.array([u0] + [so.rk_grid(4, t[i], t[i + 1], Nf, 0, q, u0) for q in range(1, Nf + 1)])
        assert np.array_equal(_bits(blk), _bits(ref)), i
    # the same by name and by a dict of t and u
    assert np.array_equal(_bits(p.build_cont_traj(list(p.runs)[0])), _bits(dense))
    assert np.array_equal(_bits(p.build_cont_traj({'t': r['t'], 'u': r['u']})), _bits(dense))


def test_build_cont_traj_every_and_times(gpu, lorenz_run):
    ode, solver, p, r, dense = lorenz_run
    N, Nf = 8, 45
    keep = [0, 10, 20, 30, 40, 45]
    sparse, ts = p.build_cont_traj(every=10, return_t=True)
    assert sparse.shape == (N * 6, 3) and ts.shape == (N * 6,)
    for i in range(N):
        assert np.array_equal(_bits(sparse[i * 6:(i + 1) * 6]), _bits(dense[i * (Nf + 1):(i + 1) * (Nf + 1)][keep])), i
        assert np.array_equal(ts[i * 6:(i + 1) * 6], np.linspace(r['t'][i], r['t'][i + 1], Nf + 1)[keep]), i
    dense2, td = p.build_cont_traj(return_t=True)
    assert np.array_equal(_bits(dense2), _bits(dense))
    assert np.array_equal(td, np.concatenate([np.linspace(r['t'][i], r['t'][i + 1], Nf + 1) for i in range(N)]))


def test_build_cont_traj_of_a_light_run(gpu, lorenz_run):
    ode, solver, p, r, dense = lorenz_run
    pl = gpu.PararealLight(ode, solver, [0, 4], 8, verbose=None)
    rl = pl.run(model='parareal', early_stop=2)
    assert rl['u'].ndim == 2 and rl['u'].shape == (9, 3)   # the newest iterate only
    light = pl.build_cont_traj()
    assert light.shape == dense.shape and np.all(np.isfinite(light))
    for i in range(8):
        assert np.array_equal(_bits(light[i * 46]), _bits(rl['u'][i])), i
    # the same iterate as the last column of a 3-D history, through the full driver
    same = p.build_cont_traj({'t': rl['t'], 'u': np.ascontiguousarray(rl['u'][:, :, None])})
    assert np.array_equal(_bits(light), _bits(same))
    sparse = pl.build_cont_traj(every=10)
    assert np.array_equal(_bits(sparse), _bits(light.reshape(8, 46, 3)[:, [0, 10, 20, 30, 40, 45]].reshape(-1, 3)))
