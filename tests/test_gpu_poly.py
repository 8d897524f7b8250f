"""PolyODE on the GPU: the lane form (d <= 4 and at most 16 terms, the table in the kernel
arguments) and the field form (everything else up to d = 2048, the table in device memory) against
the NumPy restatement of the arithmetic contract (tests/poly_ref.py, validated on the CPU by
tests/test_poly_host.py) bit for bit; Brusselator written as monomials against the built-in,
oracle-pinned Brusselator bit for bit through every driver surface; and whole runs against the
reference's recorded ones (tests/golden/poly.npz).

7 steps everywhere (odd: the remainder of any unrolled step loop is taken).  Inputs hold no exact
zero (the contract leaves the sign of a zero sum open; `==` ignores it).

Shapes.  Lane form: d = 1 (logistic), 2 (Brusselator), 3 (Lorenz; the Hopf normal form, 9 terms;
an empty and a constant-only row), 4 with exactly 16 terms (the cap); 1, 63, 64, 65 and 300 slices
(a partial wave, a full one, one lane more, several blocks).  Field form: the same d = 4 system
plus one term (17), and Lorenz-96 at d = 5, 40 (one partial wave), 256, 257 (4 / 5 whole waves, one
element per thread), 1024, 1025 (one element per thread / 8 per thread in 256 threads), 2048 (the
ceiling); 1, 5 and 300 slices (at d = 1024, 300 slices switch to two elements per thread)."""
import numpy as np
import pytest

from conftest import golden
from poly_ref import BRUS, SMALL, VDP, L96_BOUNDS, PolyNP, lorenz96, rk_np, spans, states

pytestmark = pytest.mark.gpu
TABS = ['RK1', 'RK2', 'RK4', 'RK8']
L96_D = [5, 40, 256, 257, 1024, 1025, 2048]
CASES = list(SMALL) + L96_D


def _t(torch, a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device='cuda')


def _rows(case):
    if isinstance(case, str):
        rows, centre, _, (mn, mx) = SMALL[case]
        return rows, np.array(centre), mn, mx
    return lorenz96(case), np.full(case, 2.0), L96_BOUNDS[0], L96_BOUNDS[1]


_CACHE = {}


def _pair(gpu, case, norm):
    """(PolyODE, its NumPy restatement), one table per (case, norm) for the whole module"""
    key = (case, norm)
    if key not in _CACHE:
        rows, centre, mn, mx = _rows(case)
        if norm:
            ode = gpu.PolyODE(rows, centre, mn=mn, mx=mx, normalization='-11')
            _CACHE[key] = (ode, PolyNP(rows, mn, mx))
        else:
            _CACHE[key] = (gpu.PolyODE(rows, centre), PolyNP(rows))
    return _CACHE[key]


def _seed(case):
    return CASES.index(case)


@pytest.mark.parametrize('case', CASES)
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
    T0, T1 = spans(5)
    for norm in (False, True):
        ode, ref = _pair(gpu, case, norm)
        U0 = states(case, 5, 100 + _seed(case), norm)
        for mode in ('fixed', 'linspace'):
            s = gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=7, F=tab, G='RK1', step_mode=mode)
            got = s.run_F_batch(_t(torch, T0), _t(torch, T1), _t(torch, U0)).cpu().numpy()
            want = rk_np(ref, int(tab[2:]), T0, T1, 7, U0, mode)
            assert np.all(np.isfinite(got)) and np.array_equal(got, want), (norm, mode)


@pytest.mark.parametrize('case,n', [(c, n) for c in ('brus', 'd4_16') for n in (1, 63, 64, 65, 300)] +
                         [(c, n) for c in ('d4_17', 40, 257, 1024) for n in (1, 5, 300)])
def test_slice_counts(gpu, case, n):
    import torch
    ode, ref = _pair(gpu, case, True)
    U0 = states(case, n, 7 * n + _seed(case), True)
    T0, T1 = spans(n)
    for tab, mode in (('RK4', 'fixed'), ('RK2', 'linspace')):
        s = gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=7, F=tab, G='RK1', step_mode=mode)
        got = s.run_F_batch(_t(torch, T0), _t(torch, T1), _t(torch, U0)).cpu().numpy()
        assert np.array_equal(got, rk_np(ref, int(tab[2:]), T0, T1, 7, U0, mode)), (tab, mode)


@pytest.mark.parametrize('case', ['hopf_nf', 'd4_17', 257])
def test_rk_batch_grid_walks_the_global_grid(gpu, case):
    import ctypes
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


def _grid_prefix(torch, ode, tab, T0, T1, U0, k):
    """the end state after the first k steps of the 7-step linspace grid (nngp_rk_batch_grid)"""
    import ctypes
    from nngp_amd import _lib
    out = torch.empty_like(U0)
    j0 = torch.zeros(U0.shape[0], dtype=torch.int64, device='cuda')
    cs = ode.get_vector_field().csystem(U0.device)
    _lib.check(_lib.lib().nngp_rk_batch_grid(ctypes.byref(cs), int(tab[2:]), U0.shape[0], T0.data_ptr(), T1.data_ptr(),
                                             7, j0.data_ptr(), k, U0.data_ptr(), out.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream))
    return out


@pytest.mark.parametrize('case', ['lorenz', 'd4_17', 257, 1025])
@pytest.mark.parametrize('tab', ['RK1', 'RK4', 'RK8'])
def test_trajectory_rows_are_the_end_states_after_that_many_steps(gpu, case, tab):
    """every = 1: row k is the end state of the grid's first k steps (linspace) and the last row is
    run_F_batch's end state (both modes); every = 3, 7: the rows min(p*every, 7) of every = 1"""
    import torch
    ode, _ = _pair(gpu, case, True)
    U0 = _t(torch, states(case, 5, 11, True))
    T0, T1 = spans(5)
    T0, T1 = _t(torch, T0), _t(torch, T1)
    for mode in ('fixed', 'linspace'):
        s = gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=7, F=tab, G='RK1', step_mode=mode)
        full = s.run_F_traj_batch(T0, T1, U0, every=1)
        assert full.shape[1] == 8 and torch.equal(full[:, 0], U0)
        assert torch.equal(full[:, 7], s.run_F_batch(T0, T1, U0))
        if mode == 'linspace':
            for k in range(1, 8):
                assert torch.equal(full[:, k], _grid_prefix(torch, ode, tab, T0, T1, U0, k)), k
        for every, rows in ((3, [0, 3, 6, 7]), (7, [0, 7])):
            assert torch.equal(s.run_F_traj_batch(T0, T1, U0, every=every), full[:, rows]), (mode, every)


@pytest.mark.parametrize('case', ['brus', 'd4_16', 'd4_17', 40, 1025])
def test_trajectory_rows_are_bitwise_the_numpy_stepper(gpu, case):
    """row p against min(3p, 7) steps of the stepper on the launch's own grid of 7 steps"""
    import torch
    ode, ref = _pair(gpu, case, False)
    U0 = states(case, 5, 13, False)
    T0, T1 = spans(5)
    for mode in ('fixed', 'linspace'):
        s = gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=7, F='RK4', G='RK1', step_mode=mode)
        traj = s.run_F_traj_batch(_t(torch, T0), _t(torch, T1), _t(torch, U0), every=3).cpu().numpy()
        assert np.array_equal(traj[:, 0], U0)
        for p, k in ((1, 3), (2, 6), (3, 7)):
            assert np.array_equal(traj[:, p], rk_np(ref, 4, T0, T1, k, U0, mode, gsteps=7)), (mode, p)


@pytest.mark.parametrize('case', ['hopf_nf', 'd4_16', 'd4_17', 40, 1025])
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
    for a, b in (('brus', 'hopf_nf'), ('d4_17', 40)):      # two lane tables, two field tables
        (oa, ra), (ob, rb) = _pair(gpu, a, False), _pair(gpu, b, False)
        assert oa.nx != ob.nx
        sa = gpu.SolverRK(oa.get_vector_field(), Ng=1, Nf=7, F='RK4', G='RK1')
        sb = gpu.SolverRK(ob.get_vector_field(), Ng=1, Nf=7, F='RK4', G='RK1')
        Ua, Ub = states(a, 5, 1, False), states(b, 5, 2, False)
        wa, wb = rk_np(ra, 4, T0, T1, 7, Ua), rk_np(rb, 4, T0, T1, 7, Ub)
        for _ in range(3):
            assert np.array_equal(sa.run_F_batch(t0, t1, _t(torch, Ua)).cpu().numpy(), wa)
            assert np.array_equal(sb.run_F_batch(t0, t1, _t(torch, Ub)).cpu().numpy(), wb)


@pytest.mark.parametrize('rows,u0', [(BRUS, [1.0, 3.07]), (lorenz96(40), np.full(40, 2.0))])
def test_a_destroyed_table_is_refused(gpu, rows, u0):
    import torch
    ode = gpu.PolyODE(rows, u0)
    s = gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=7, F='RK4', G='RK1')
    U0 = _t(torch, np.array(u0)[None, :] + 0.125)
    t0, t1 = _t(torch, [0.0]), _t(torch, [0.01])
    assert torch.all(torch.isfinite(s.run_F_batch(t0, t1, U0)))
    ode.destroy()
    with pytest.raises(gpu.NNGPError, match='poly'):
        s.run_F_batch(t0, t1, U0)
    with pytest.raises(gpu.NNGPError, match='poly'):
        s.run_F_traj_batch(t0, t1, U0)
    with pytest.raises(gpu.NNGPError, match='poly'):
        s.f(0.0, np.array(u0) + 0.125)


# ------------------------------------------------------------------------------------------------
# Brusselator as monomials is the built-in Brusselator, bit for bit, through every surface
# ------------------------------------------------------------------------------------------------
BRUS_MN, BRUS_MX = [0.4, 0.9], [4.0, 5.0]


def _brus_pair(gpu, norm):
    if norm:
        return gpu.PolyODE(BRUS, [1, 3.07], mn=BRUS_MN, mx=BRUS_MX, normalization='-11'), \
            gpu.Brusselator(normalization='-11')
    return gpu.PolyODE(BRUS, [1, 3.07]), gpu.Brusselator()


@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('tab', TABS)
def test_brusselator_rows_are_bitwise_the_builtin_propagators(gpu, norm, tab):
    import torch
    poly, built = _brus_pair(gpu, norm)
    U0 = _t(torch, states('brus', 65, 17, norm))
    T0, T1 = spans(65)
    T0, T1 = _t(torch, T0), _t(torch, T1)
    assert np.array_equal(poly.get_vector_field()(0.0, U0.cpu().numpy()),
                          built.get_vector_field()(0.0, U0.cpu().numpy()))
    for mode in ('fixed', 'linspace'):
        sp = gpu.SolverRK(poly.get_vector_field(), Ng=3, Nf=7, F=tab, G=tab, step_mode=mode)
        sb = gpu.SolverRK(built.get_vector_field(), Ng=3, Nf=7, F=tab, G=tab, step_mode=mode)
        assert torch.equal(sp.run_F_batch(T0, T1, U0), sb.run_F_batch(T0, T1, U0))
        assert torch.equal(sp.run_G_batch(T0, T1, U0), sb.run_G_batch(T0, T1, U0))
        for every in (1, 3, 7):
            assert torch.equal(sp.run_F_traj_batch(T0, T1, U0, every=every),
                               sb.run_F_traj_batch(T0, T1, U0, every=every))


def _same(a, b):
    return np.array_equal(np.nan_to_num(a, nan=7.0), np.nan_to_num(b, nan=7.0))


@pytest.fixture(scope='module')
def brus_nngp(gpu):
    """nnGParareal on the built-in Brusselator, nn = 10, seed 45, speculation off: shared, unchanged"""
    ode = gpu.Brusselator(normalization='-11')
    s = gpu.SolverRK(ode.get_vector_field(), Ng=4, Nf=40, F='RK4', G='RK1')
    r = gpu.Parareal(ode, s, [0, 12], 16, epsilon=5e-7, verbose=None, speculate=0).run(model='nngp', nn=10, seed=45)
    r['u'].setflags(write=False)
    return r


@pytest.mark.parametrize('speculate', [0, 1])
def test_brusselator_rows_give_the_builtin_nngparareal_run(gpu, brus_nngp, speculate):
    """The built-in runs G inside the sweep's kernels, the new kind by launches: the same bits."""
    ode = gpu.PolyODE(BRUS, [1, 3.07], mn=BRUS_MN, mx=BRUS_MX, normalization='-11')
    s = gpu.SolverRK(ode.get_vector_field(), Ng=4, Nf=40, F='RK4', G='RK1')
    r = gpu.Parareal(ode, s, [0, 12], 16, epsilon=5e-7, verbose=None, speculate=speculate).run(
        model='nngp', nn=10, seed=45)
    assert brus_nngp['converged'] and r['converged']
    assert r['k'] == brus_nngp['k'] and r['conv_int'] == brus_nngp['conv_int'] and _same(r['u'], brus_nngp['u'])


# ------------------------------------------------------------------------------------------------
# whole runs against the reference's recorded ones
# ------------------------------------------------------------------------------------------------
def _parareal(gpu, key, **kw):
    R = golden('poly.npz')
    _, T, N, Ng, Nf, eps, g_order = R[f'para__{key}__cfg']
    if key == 'vdp':
        ode = gpu.PolyODE(VDP, [2.0, 0.0], mn=[-2.5, -3.0], mx=[2.5, 3.0], normalization='-11', name='VanDerPol')
    else:
        ode = gpu.PolyODE(lorenz96(40), 8.0 + 0.5 * np.sin(1.0 + 2.0 * np.arange(40)), mn=L96_BOUNDS[0],
                          mx=L96_BOUNDS[1], normalization='-11', name='Lorenz96_40')
    assert np.array_equal(ode.get_init_cond(), R[f'init__{key}_n__u0'])
    s = gpu.SolverRK(ode.get_vector_field(), Ng=int(Ng), Nf=int(Nf), F='RK4', G=f'RK{int(g_order)}')
    return gpu.Parareal(ode, s, [0, float(T)], int(N), epsilon=float(eps), verbose=None, **kw)


def _final(u):
    """the last computed iterate of a reference `u` [N+1][d][iterations] (NaN where not computed)"""
    cols = [c for c in range(u.shape[2]) if not np.any(np.isnan(u[:, :, c]))]
    return u[:, :, cols[-1]]


def _bound(R, key):
    """max(10 eps, 10 x the classic run's own distance from the serial fine solution): the models
    stop on the same eps = 5e-7 but along different iterates"""
    return max(5e-6, 10 * np.max(np.abs(_final(R[f'para__{key}__u']) - R[f'para__{key}__fine'])))


@pytest.mark.parametrize('key', ['vdp', 'l96'])
def test_classic_parareal_matches_reference(gpu, key):
    R = golden('poly.npz')
    r = _parareal(gpu, key).run(model='parareal')
    assert r['converged']
    assert r['k'] == int(R[f'para__{key}__k'])
    assert r['conv_int'] == list(R[f'para__{key}__conv_int'])
    assert np.nanmax(np.abs(r['u'] - R[f'para__{key}__u'])) < 1e-9


@pytest.mark.parametrize('model,kw', [('nngp', dict(nn=10, seed=45)), ('elm', {}), ('gpjax', {})])
def test_learned_models_converge_to_the_fine_solution(gpu, model, kw):
    R = golden('poly.npz')
    r = _parareal(gpu, 'vdp').run(model=model, **kw)
    assert r['converged'] and r['k'] <= 16
    assert np.max(np.abs(r['u'][:, :, -1] - R['para__vdp__fine'])) <= _bound(R, 'vdp')
