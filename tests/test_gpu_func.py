"""FuncODE on the GPU: the lane form (d <= 4, at most 4 atoms and 16 terms, the table in the kernel
arguments) and the field form (everything else up to d = n_atoms = 2048, the table in device memory,
the atoms in the tail of the stage image) against the NumPy restatement of the arithmetic contract
(tests/func_ref.py, validated on the CPU by tests/test_func_host.py) bit for bit; ThomasLabyrinth
written as three sine atoms against the built-in, oracle-pinned ThomasLabyrinth bit for bit through
every driver surface; a system without atoms against PolyODE bit for bit; and whole runs against the
reference's recorded ones (tests/golden/func.npz).

7 steps everywhere unless stated (odd: the remainder of any unrolled step loop is taken).  Inputs
hold no exact zero (the contract leaves the sign of a zero sum open; `==` ignores it).

Shapes.  Lane form: D = 1..4 with 0, 1 and 4 atoms, the 4-atom tables with exactly 16 terms (the
caps), the atoms starting at sin and at exp so that all six functions and all four argument shapes
run in the lane form; the pendulum (sin), its cosine twin, the chemostat (recip) and Gompertz with
the tanks (log, sqrt); 1, 63, 64, 65 and 300 slices.  Lane -> field fall-over: D = 4 with 5 atoms, and
with 17 terms.  Field form (d, n_atoms): (5, 1), (40, 130) one partial wave and three atoms per
thread, (256, 256), (257, 3) 4 / 5 whole waves, (1025, 1025) 8 elements per thread, (2048, 2048) the
ceiling (two 32 KB images; 2 steps); Kuramoto (8, 56), sine-Gordon (64, 32), Bratu (40, 40)."""
import ctypes

import numpy as np
import pytest

import adaptive_ref as AR
from conftest import golden
from func_ref import (GOLDEN_PARA, GOLDEN_SYSTEMS, THOMAS_ATOMS, THOMAS_BOUNDS, THOMAS_ROWS, THOMAS_U0, FuncNP,
                      n_terms, synthetic, synthetic_states)
from poly_ref import BRUS, rk_np, spans

pytestmark = pytest.mark.gpu
TABS = ['RK1', 'RK2', 'RK4', 'RK8']

# name -> (d, n_atoms, keyword arguments of func_ref.synthetic)
_LANE16 = {1: [16], 2: [8, 8], 3: [6, 5, 5], 4: [4, 4, 4, 4]}
SYNTH = {}
for _D in (1, 2, 3, 4):
    SYNTH[f'lane{_D}_a0'] = (_D, 0, {})
    SYNTH[f'lane{_D}_a1'] = (_D, 1, dict(shift=_D))
    SYNTH[f'lane{_D}_a4_t16'] = (_D, 4, dict(rows_terms=_LANE16[_D], shift=2 * (_D % 2)))
SYNTH['fall_a5'] = (4, 5, dict(shift=1))
SYNTH['fall_t17'] = (4, 4, dict(rows_terms=[5, 4, 4, 4], shift=3))
for _d, _na in ((5, 1), (40, 130), (256, 256), (257, 3), (1025, 1025)):
    SYNTH[f'field{_d}_{_na}'] = (_d, _na, {})
LANE = [k for k in SYNTH if k.startswith('lane')]
CASES = list(SYNTH) + list(GOLDEN_SYSTEMS)


def _t(torch, a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device='cuda')


_SYS = {}


def system(case):
    """the case's description (func_ref): atoms, rows, u0, mn, mx, spread"""
    if case not in _SYS:
        if case in SYNTH:
            d, na, kw = SYNTH[case]
            _SYS[case] = synthetic(d, na, **kw)
        elif case == 'ceiling':
            _SYS[case] = synthetic(2048, 2048)
        else:
            _SYS[case] = GOLDEN_SYSTEMS[case]()
    return _SYS[case]


def reference(case, norm):
    S = system(case)
    return FuncNP(S['atoms'], S['rows'], S['mn'], S['mx']) if norm else FuncNP(S['atoms'], S['rows'])


def states(case, n, seed, norm):
    return synthetic_states(system(case), n, seed, norm)


def case_spans(case, n):
    """poly_ref.spans, shortened for a stiff system (Bratu: explicit steps need h < 2 / (4 (d+1)^2))"""
    T0, T1 = spans(n)
    return T0, T0 + system(case).get('tscale', 1.0) * (T1 - T0)


_CACHE = {}


def _pair(gpu, case, norm):
    """(FuncODE, its NumPy restatement), one table per (case, norm) for the whole module"""
    key = (case, norm)
    if key not in _CACHE:
        S = system(case)
        kw = dict(mn=S['mn'], mx=S['mx'], normalization='-11') if norm else {}
        _CACHE[key] = (gpu.FuncODE(atoms=S['atoms'], terms=S['rows'], u0=S['u0'], **kw), reference(case, norm))
    return _CACHE[key]


def _seed(case):
    return (CASES + ['ceiling']).index(case)


def test_the_cases_take_the_forms_they_are_named_for():
    for case in CASES + ['ceiling']:
        S = system(case)
        d, na, nt = len(S['rows']), len(S['atoms']), n_terms(S['rows'])
        lane = d <= 4 and na <= 4 and nt <= 16
        if case.startswith('lane') or case in ('pendulum', 'pendulum_cos', 'chemostat', 'gompertz'):
            assert lane, case
        else:
            assert not lane, case
        if case.endswith('_t16'):
            assert nt == 16
    assert n_terms(system('fall_t17')['rows']) == 17 and len(system('fall_a5')['atoms']) == 5
    lane_fns = {a[0] for c in CASES for a in system(c)['atoms'] if c.startswith('lane')}
    field_fns = {a[0] for c in CASES for a in system(c)['atoms'] if c.startswith('field')}
    assert lane_fns == field_fns == {'sin', 'cos', 'exp', 'log', 'recip', 'sqrt'}


@pytest.mark.parametrize('case', CASES + ['ceiling'])
@pytest.mark.parametrize('norm', [False, True])
def test_rhs_is_bitwise_the_contract(gpu, case, norm):
    ode, ref = _pair(gpu, case, norm)
    f = ode.get_vector_field()
    U = states(case, 4, _seed(case), norm)
    got = f(0.0, U)
    assert np.all(np.isfinite(got)) and np.array_equal(got, ref(U))
    assert np.array_equal(f(0.0, U[1]), ref(U[1]))


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('tab', TABS)
def test_rk_is_bitwise_the_numpy_stepper(gpu, case, tab):
    """5 slices with their own spans; both step modes, with and without '-11'"""
    import torch
    T0, T1 = case_spans(case, 5)
    for norm in (False, True):
        ode, ref = _pair(gpu, case, norm)
        U0 = states(case, 5, 100 + _seed(case), norm)
        for mode in ('fixed', 'linspace'):
            s = gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=7, F=tab, G='RK1', step_mode=mode)
            got = s.run_F_batch(_t(torch, T0), _t(torch, T1), _t(torch, U0)).cpu().numpy()
            want = rk_np(ref, int(tab[2:]), T0, T1, 7, U0, mode)
            assert np.all(np.isfinite(got)) and np.array_equal(got, want), (norm, mode)


@pytest.mark.parametrize('tab', TABS)
def test_the_ceiling_d_2048_with_2048_atoms(gpu, tab):
    """two steps; the stage images are the 64 KB the form allows"""
    import torch
    T0, T1 = spans(2)
    for norm, mode in ((False, 'linspace'), (True, 'fixed')):
        ode, ref = _pair(gpu, 'ceiling', norm)
        U0 = states('ceiling', 2, 31, norm)
        s = gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=2, F=tab, G='RK1', step_mode=mode)
        got = s.run_F_batch(_t(torch, T0), _t(torch, T1), _t(torch, U0)).cpu().numpy()
        assert np.all(np.isfinite(got)) and np.array_equal(got, rk_np(ref, int(tab[2:]), T0, T1, 2, U0, mode))


@pytest.mark.parametrize('case,n', [(c, n) for c in ('lane2_a1', 'lane4_a4_t16', 'lane3_a4_t16', 'field257_3')
                                    for n in (1, 63, 64, 65, 300)] +
                         [(c, n) for c in ('fall_a5', 'field40_130') for n in (1, 65, 300)])
def test_slice_counts(gpu, case, n):
    import torch
    ode, ref = _pair(gpu, case, True)
    U0 = states(case, n, 7 * n + _seed(case), True)
    T0, T1 = spans(n)
    for tab, mode in (('RK4', 'fixed'), ('RK2', 'linspace')):
        s = gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=7, F=tab, G='RK1', step_mode=mode)
        got = s.run_F_batch(_t(torch, T0), _t(torch, T1), _t(torch, U0)).cpu().numpy()
        assert np.array_equal(got, rk_np(ref, int(tab[2:]), T0, T1, 7, U0, mode)), (tab, mode)


GRID_CASES = ['lane1_a4_t16', 'lane2_a4_t16', 'lane3_a1', 'lane4_a4_t16', 'gompertz', 'field257_3']


@pytest.mark.parametrize('case', GRID_CASES)
def test_rk_batch_grid_walks_the_global_grid(gpu, case):
    import torch
    from nngp_amd import _lib
    ode, ref = _pair(gpu, case, True)
    U0 = states(case, 5, 3, True)
    G0, G1 = spans(5)
    G1 = G0 + 4 * (G1 - G0)
    J0 = np.array([0, 3, 7, 14, 21])     # the last slice ends on the grid's last point
    out = torch.empty((5, U0.shape[1]), dtype=torch.float64, device='cuda')
    g0, g1, j0, u0 = _t(torch, G0), _t(torch, G1), _t(torch, J0, torch.int64), _t(torch, U0)
    cs = ode.get_vector_field().csystem(u0.device)
    _lib.check(_lib.lib().nngp_rk_batch_grid(ctypes.byref(cs), 4, 5, g0.data_ptr(), g1.data_ptr(), 28, j0.data_ptr(),
                                             7, u0.data_ptr(), out.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream))
    want = np.array([rk_np(ref, 4, G0[i], G1[i], 7, U0[i], 'linspace', gsteps=28, j0=int(J0[i])) for i in range(5)])
    assert np.array_equal(out.cpu().numpy(), want)


def _grid_prefix(torch, ode, tab, T0, T1, U0, k, steps):
    """the end state after the first k steps of the `steps`-step linspace grid (nngp_rk_batch_grid)"""
    from nngp_amd import _lib
    out = torch.empty_like(U0)
    j0 = torch.zeros(U0.shape[0], dtype=torch.int64, device='cuda')
    cs = ode.get_vector_field().csystem(U0.device)
    _lib.check(_lib.lib().nngp_rk_batch_grid(ctypes.byref(cs), int(tab[2:]), U0.shape[0], T0.data_ptr(), T1.data_ptr(),
                                             steps, j0.data_ptr(), k, U0.data_ptr(), out.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream))
    return out


@pytest.mark.parametrize('case', GRID_CASES)
@pytest.mark.parametrize('tab', ['RK1', 'RK4', 'RK8'])
def test_trajectory_rows_are_the_end_states_after_that_many_steps(gpu, case, tab):
    """12 steps.  every = 1: row k is bitwise the stepper's state after k steps of the launch's own
    grid (both modes), the grid launch's prefix (linspace), and the last row run_F_batch's end state;
    every = 5: the rows 0, 5, 10, 12 of every = 1"""
    import torch
    ode, ref = _pair(gpu, case, True)
    U = states(case, 5, 11, True)
    U0 = _t(torch, U)
    T0n, T1n = spans(5)
    T0, T1 = _t(torch, T0n), _t(torch, T1n)
    for mode in ('fixed', 'linspace'):
        s = gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=12, F=tab, G='RK1', step_mode=mode)
        full = s.run_F_traj_batch(T0, T1, U0, every=1)
        assert full.shape[1] == 13 and torch.equal(full[:, 0], U0)
        assert torch.equal(full[:, 12], s.run_F_batch(T0, T1, U0))
        for k in (1, 5, 12):
            assert np.array_equal(full[:, k].cpu().numpy(), rk_np(ref, int(tab[2:]), T0n, T1n, k, U, mode, gsteps=12)), k
        if mode == 'linspace':
            for k in range(1, 13):
                assert torch.equal(full[:, k], _grid_prefix(torch, ode, tab, T0, T1, U0, k, 12)), k
        assert torch.equal(s.run_F_traj_batch(T0, T1, U0, every=5), full[:, [0, 5, 10, 12]]), mode


# ------------------------------------------------------------------------------------------------
# the adaptive propagator
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['pendulum', 'sinegordon'])
@pytest.mark.parametrize('method', ['RK23', 'RK45'])
@pytest.mark.parametrize('first_step', [0.0, 0.01])
def test_adaptive_is_bitwise_the_restatement(gpu, case, method, first_step):
    """lane form (pendulum) and field form (sine-Gordon, d = 64): end states and the statistics"""
    import torch
    from nngp_amd import _lib
    n, nf, rtol, atol = 3, 4, 1e-5, 1e-8
    for norm in (False, True):
        ode, ref = _pair(gpu, case, norm)
        U0 = states(case, n, 41, norm)
        T0 = 0.25 + 0.0625 * np.arange(n)
        T1 = T0 + 0.3 + 0.05 * np.arange(n)
        want, wstats = AR.solve_batch(ref, method, T0, T1, nf, U0, rtol=rtol, atol=atol,
                                      first_step=first_step or None)
        assert np.all(wstats[:, 0] == 0) and np.all(wstats[:, 2] >= 2)
        t0, t1, u0 = _t(torch, T0), _t(torch, T1), _t(torch, U0)
        uF = torch.empty_like(u0)
        stats = torch.full((n, 4), -7, dtype=torch.int64, device='cuda')
        cs = ode.get_vector_field().csystem(u0.device)
        _lib.check(_lib.lib().nngp_rk_adaptive(ctypes.byref(cs), AR.METHOD_CODE[method], n, t0.data_ptr(), t1.data_ptr(),
                                               nf, rtol, atol, first_step, 100 * nf + 1000, u0.data_ptr(),
                                               uF.data_ptr(), stats.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream))
        assert np.array_equal(uF.cpu().numpy(), want), norm
        assert np.array_equal(stats.cpu().numpy(), wstats), norm


# ------------------------------------------------------------------------------------------------
# ThomasLabyrinth as three sine atoms is the built-in ThomasLabyrinth, bit for bit, through every surface
# ------------------------------------------------------------------------------------------------
def _thomas_pair(gpu, norm):
    kw = dict(mn=THOMAS_BOUNDS[0], mx=THOMAS_BOUNDS[1], normalization='-11') if norm else {}
    return (gpu.FuncODE(atoms=THOMAS_ATOMS, terms=THOMAS_ROWS, u0=THOMAS_U0, **kw),
            gpu.ThomasLabyrinth(**(dict(normalization='-11') if norm else {})))


def _thomas_states(n, seed, norm):
    U = np.random.default_rng(seed).uniform(-11, 11, (n, 3))
    return U / 12.0 if norm else U


@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('tab', TABS)
def test_thomas_rows_are_bitwise_the_builtin_propagators(gpu, norm, tab):
    import torch
    func, built = _thomas_pair(gpu, norm)
    U0 = _t(torch, _thomas_states(65, 17, norm))
    T0, T1 = spans(65)
    T0, T1 = _t(torch, T0), _t(torch, T1)
    assert np.array_equal(func.get_vector_field()(0.0, U0.cpu().numpy()),
                          built.get_vector_field()(0.0, U0.cpu().numpy()))
    for mode in ('fixed', 'linspace'):
        sf = gpu.SolverRK(func.get_vector_field(), Ng=3, Nf=7, F=tab, G=tab, step_mode=mode)
        sb = gpu.SolverRK(built.get_vector_field(), Ng=3, Nf=7, F=tab, G=tab, step_mode=mode)
        assert torch.equal(sf.run_F_batch(T0, T1, U0), sb.run_F_batch(T0, T1, U0))
        assert torch.equal(sf.run_G_batch(T0, T1, U0), sb.run_G_batch(T0, T1, U0))
        for every in (1, 5):
            assert torch.equal(sf.run_F_traj_batch(T0, T1, U0, every=every),
                               sb.run_F_traj_batch(T0, T1, U0, every=every))


@pytest.mark.parametrize('norm', [False, True])
def test_thomas_rows_are_bitwise_the_builtin_adaptive_solver(gpu, norm):
    import torch
    func, built = _thomas_pair(gpu, norm)
    U0 = _t(torch, _thomas_states(5, 19, norm))
    T0, T1 = spans(5)
    T0, T1 = _t(torch, T0), _t(torch, T0 + 20 * (T1 - T0))
    sf = gpu.SolverScipy(func.get_vector_field(), 1, 4, 'RK1', F='RK45', rtol=1e-6, atol=1e-9)
    sb = gpu.SolverScipy(built.get_vector_field(), 1, 4, 'RK1', F='RK45', rtol=1e-6, atol=1e-9)
    assert torch.equal(sf.run_F_batch(T0, T1, U0), sb.run_F_batch(T0, T1, U0))
    for key in ('status', 'nfev', 'n_accepted', 'n_rejected'):
        assert np.array_equal(sf.last_stats[key], sb.last_stats[key]), key


def _same(a, b):
    return np.array_equal(np.nan_to_num(a, nan=7.0), np.nan_to_num(b, nan=7.0))


@pytest.fixture(scope='module')
def thomas_nngp(gpu):
    """nnGParareal on the built-in ThomasLabyrinth, nn = 10, seed 45, speculation off: shared, unchanged"""
    ode = gpu.ThomasLabyrinth(normalization='-11')
    s = gpu.SolverRK(ode.get_vector_field(), Ng=4, Nf=40, F='RK4', G='RK1')
    r = gpu.Parareal(ode, s, [0, 4], 16, epsilon=5e-7, verbose=None, speculate=0).run(model='nngp', nn=10, seed=45)
    r['u'].setflags(write=False)
    return r


@pytest.mark.parametrize('speculate', [0, 1])
def test_thomas_rows_give_the_builtin_nngparareal_run(gpu, thomas_nngp, speculate):
    """The built-in runs G inside the sweep's kernels, the new kind by launches: the same bits."""
    ode = gpu.FuncODE(atoms=THOMAS_ATOMS, terms=THOMAS_ROWS, u0=THOMAS_U0, mn=THOMAS_BOUNDS[0], mx=THOMAS_BOUNDS[1],
                      normalization='-11')
    s = gpu.SolverRK(ode.get_vector_field(), Ng=4, Nf=40, F='RK4', G='RK1')
    r = gpu.Parareal(ode, s, [0, 4], 16, epsilon=5e-7, verbose=None, speculate=speculate).run(
        model='nngp', nn=10, seed=45)
    assert thomas_nngp['converged'] and r['converged']
    assert r['k'] == thomas_nngp['k'] and r['conv_int'] == thomas_nngp['conv_int'] and _same(r['u'], thomas_nngp['u'])


@pytest.mark.parametrize('norm', [False, True])
def test_zero_atom_brusselator_rows_are_bitwise_polyode(gpu, norm):
    import torch
    kw = dict(mn=[0.4, 0.9], mx=[4.0, 5.0], normalization='-11') if norm else {}
    func = gpu.FuncODE(atoms=[], terms=BRUS, u0=[1, 3.07], **kw)
    poly = gpu.PolyODE(BRUS, [1, 3.07], **kw)
    rng = np.random.default_rng(23)
    U = np.array([1.0, 3.07]) + 0.3 * rng.uniform(-1, 1, (65, 2))
    U0 = _t(torch, 2 * (U - np.array(kw['mn'])) / (np.array(kw['mx']) - np.array(kw['mn'])) - 1 if norm else U)
    T0, T1 = spans(65)
    T0, T1 = _t(torch, T0), _t(torch, T1)
    assert np.array_equal(func.get_vector_field()(0.0, U0.cpu().numpy()), poly.get_vector_field()(0.0, U0.cpu().numpy()))
    for tab in TABS:
        for mode in ('fixed', 'linspace'):
            sf = gpu.SolverRK(func.get_vector_field(), Ng=1, Nf=7, F=tab, G='RK1', step_mode=mode)
            sp = gpu.SolverRK(poly.get_vector_field(), Ng=1, Nf=7, F=tab, G='RK1', step_mode=mode)
            assert torch.equal(sf.run_F_batch(T0, T1, U0), sp.run_F_batch(T0, T1, U0)), (tab, mode)


@pytest.mark.parametrize('case', ['pendulum', 'kuramoto', 'field1025_1025'])
@pytest.mark.parametrize('tab', TABS)
def test_contracted_build_within_1e12_of_exact(gpu, case, tab):
    import torch
    ode, _ = _pair(gpu, case, True)
    U0 = _t(torch, states(case, 5, 5, True))
    T0, T1 = spans(5)
    T0, T1 = _t(torch, T0), _t(torch, T1)
    run = lambda fma: gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=40, F=tab, G='RK1',
                                   fma=fma).run_F_batch(T0, T1, U0).cpu().numpy()
    ex, fm = run(False), run(True)
    assert np.all(np.isfinite(fm))
    assert np.max(np.abs(fm - ex)) / max(1.0, np.max(np.abs(ex))) <= 1e-12


def test_two_live_tables_keep_their_own_results(gpu):
    import torch
    T0, T1 = spans(5)
    t0, t1 = _t(torch, T0), _t(torch, T1)
    for a, b in (('pendulum', 'gompertz'), ('fall_a5', 'field40_130')):      # two lane tables, two field tables
        (oa, ra), (ob, rb) = _pair(gpu, a, False), _pair(gpu, b, False)
        assert oa.nx != ob.nx
        sa = gpu.SolverRK(oa.get_vector_field(), Ng=1, Nf=7, F='RK4', G='RK1')
        sb = gpu.SolverRK(ob.get_vector_field(), Ng=1, Nf=7, F='RK4', G='RK1')
        Ua, Ub = states(a, 5, 1, False), states(b, 5, 2, False)
        wa, wb = rk_np(ra, 4, T0, T1, 7, Ua), rk_np(rb, 4, T0, T1, 7, Ub)
        for _ in range(3):
            assert np.array_equal(sa.run_F_batch(t0, t1, _t(torch, Ua)).cpu().numpy(), wa)
            assert np.array_equal(sb.run_F_batch(t0, t1, _t(torch, Ub)).cpu().numpy(), wb)


@pytest.mark.parametrize('case', ['pendulum', 'bratu'])
def test_a_destroyed_table_is_refused(gpu, case):
    import torch
    S = system(case)
    ode = gpu.FuncODE(atoms=S['atoms'], terms=S['rows'], u0=S['u0'])
    s = gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=7, F='RK4', G='RK1')
    sc = gpu.SolverScipy(s.f, 1, 4, 'RK1', F='RK45')   # the same descriptor: made before the table goes
    U0 = _t(torch, np.array(S['u0'])[None, :] + 0.015625)
    t0, t1 = _t(torch, [0.0]), _t(torch, [0.0007])
    assert torch.all(torch.isfinite(s.run_F_batch(t0, t1, U0)))
    assert torch.all(torch.isfinite(sc.run_F_batch(t0, t1, U0)))
    ode.destroy()
    with pytest.raises(gpu.NNGPError, match='func'):
        s.run_F_batch(t0, t1, U0)
    with pytest.raises(gpu.NNGPError, match='func'):
        s.run_F_traj_batch(t0, t1, U0)
    with pytest.raises(gpu.NNGPError, match='func'):
        s.f(0.0, np.array(S['u0']) + 0.015625)
    with pytest.raises(gpu.NNGPError, match='func'):
        sc.run_F_batch(t0, t1, U0)


# ------------------------------------------------------------------------------------------------
# whole runs against the reference's recorded ones
# ------------------------------------------------------------------------------------------------
def _parareal(gpu, key, **kw):
    R = golden('func.npz')
    _, T, N, Ng, Nf, eps, g_order = R[f'para__{key}__cfg']
    assert (float(T), int(N), int(Ng), int(Nf), f'RK{int(g_order)}') == GOLDEN_PARA[key]
    S = GOLDEN_SYSTEMS[key]()
    ode = gpu.FuncODE(atoms=S['atoms'], terms=S['rows'], u0=S['u0'], mn=S['mn'], mx=S['mx'], normalization='-11',
                      name=key)
    assert np.array_equal(ode.get_init_cond(), R[f'para__{key}__u0'])
    s = gpu.SolverRK(ode.get_vector_field(), Ng=int(Ng), Nf=int(Nf), F='RK4', G=f'RK{int(g_order)}')
    return gpu.Parareal(ode, s, [0, float(T)], int(N), epsilon=float(eps), verbose=None, **kw)


@pytest.mark.parametrize('key', list(GOLDEN_PARA))
def test_classic_parareal_matches_reference(gpu, key):
    """the fixture's k and conv_int; the final iterate within the fixture's own distance to its serial
    fine solution plus 1e-9"""
    R = golden('func.npz')
    r = _parareal(gpu, key).run(model='parareal')
    assert r['converged']
    assert r['k'] == int(R[f'para__{key}__k'])
    assert r['conv_int'] == list(R[f'para__{key}__conv_int'])
    own = np.max(np.abs(R[f'para__{key}__final'] - R[f'para__{key}__fine']))
    assert np.max(np.abs(r['u'][:, :, -1] - R[f'para__{key}__fine'])) <= own + 1e-9


@pytest.mark.parametrize('model,kw', [('nngp', dict(nn=10, seed=45)), ('elm', {}), ('gpjax', {})])
def test_learned_models_converge_to_the_fine_solution(gpu, model, kw):
    """the bound of tests/test_gpu_poly.py's learned-model test: max(10 eps, 10 x the classic run's own
    distance from the serial fine solution)"""
    R = golden('func.npz')
    bound = max(5e-6, 10 * np.max(np.abs(R['para__pendulum__final'] - R['para__pendulum__fine'])))
    r = _parareal(gpu, 'pendulum').run(model=model, **kw)
    assert r['converged'] and r['k'] <= 8
    assert np.max(np.abs(r['u'][:, :, -1] - R['para__pendulum__fine'])) <= bound
