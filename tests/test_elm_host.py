"""CPU: the ELM arithmetic contract's NumPy restatement (tests/elm_ref.py) against the reference's
own ELM_base (tests/golden/elm.npz and elm_wide.npz, written by tests/golden/gen_elm.py), and the ELM surface's
refusals and argument checks, none of which needs a GPU.

Tolerances.  The restatement is a min-norm solve on differences, the reference a
Ridge(alpha=0) through the Gram of the centred rows: they agree where the Gram is well conditioned.
That is a statement about the formulation, so it is checked at the threshold's starting value
elm_ref.TAU_EXACT = 2^-52, where only rows the reference's own arithmetic has lost are dropped.  The
model's threshold elm_ref.TAU = 2^-8 (the value the convergence condition below asks for) drops
neighbours the reference keeps: there the restatement is held to the exact formulation bit for bit
wherever it drops no further row, and differs from the reference by O(1) where it does (10 of the
150 well-conditioned fixture cases; the first correction of both whole runs).
Measured with the restatement at TAU_EXACT on the development CPU, relative to max(1, |ref|):
  predictions, fixture cases with cond <= 1e6 (150 of 160):   9.49e-13   -> bound 100 x = 9.49e-11
  wide layers (tests/golden/elm_wide.npz: res_size 500 at degree 2, 200 and 100 at degree 1, m = 5, 10,
  16, 40 training rows), cond <= 1e6 (90 of 90, largest 3.4e4): 8.63e-13   -> bound 100 x = 8.63e-11
  (the model's TAU drops a further neighbour in 13 of those 90)
  whole run, column 1 (the first correction), Lorenz N = 32:  2.96e-10   -> bound 100 x = 2.96e-8
  whole run, column 1, FHN-ODE N = 40:                        2.74e-12   -> bound 100 x = 2.74e-10
The factor 100 covers BLAS / sklearn builds that order their sums differently; the GPU gets no
margin, it is held to the restatement bit for bit (tests/test_gpu_elm.py).
"""
import ctypes

import numpy as np
import pytest

import elm_ref as E
from conftest import golden
from elm_cases import EPS, RUNS, cpu_loop, serial_fine

WEIGHTS = ((2, 20, 2), (3, 20, 2), (3, 7, 1), (16, 50, 2))   # (d, res_size, degree) of the fixture
MS = (1, 2, 4, 7)
COND_MAX = 1e6
PRED_MEASURED, PRED_BOUND = 9.49e-13, 100 * 9.49e-13
WIDE_WEIGHTS = ((3, 500, 2), (16, 200, 1), (3, 100, 1))   # of tests/golden/elm_wide.npz
WIDE_MS = (5, 10, 16)
WIDE_MEASURED, WIDE_BOUND = 8.63e-13, 100 * 8.63e-13
COL1 = {'lorenz': (2.96e-10, 100 * 2.96e-10), 'fhn_ode': (2.74e-12, 100 * 2.74e-12)}   # measured, bound


@pytest.mark.parametrize('d,res,deg', WEIGHTS)
def test_weights_equal_the_reference_bitwise(d, res, deg):
    z = golden('elm.npz')
    tag = f'w__{d}_{res}_{deg}'
    bias, C = E.draw_weights(d, 47, res, deg)
    assert C.shape == (res, E.n_poly(d, deg))
    assert np.array_equal(bias, z[tag + '__bias'][:, 0]) and np.array_equal(C, z[tag + '__C'])


def test_feature_order_is_sklearns():
    x = np.array([2.0, 3.0, 5.0])
    assert E.features(x, 2).tolist() == [1, 2, 3, 5, 4, 6, 10, 9, 15, 25]
    assert E.features(x, 1).tolist() == [1, 2, 3, 5]
    assert E.feature_pairs(3) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def _compare_predictions(z, weights, ms):
    """(largest relative difference at TAU_EXACT, cases compared, cases in all, cases where the model's
    TAU drops a further neighbour) over the fixture z; asserts the model-threshold property."""
    worst, under, total, dropped = 0.0, 0, 0, 0
    for d, res, deg in weights:
        tag = f'w__{d}_{res}_{deg}'
        X, Y, Q = z[tag + '__X'], z[tag + '__Y'], z[tag + '__Q']
        for m in ms:
            ref, cond = z[tag + f'__pred_m{m}'], z[tag + f'__cond_m{m}']
            for c in range(X.shape[0]):
                total += 1
                if not cond[c] <= COND_MAX:
                    continue
                under += 1
                mdl = E.ElmRef(d, 47, res, 1, deg, m, tau=E.TAU_EXACT)
                mdl.fit(X[c], Y[c])
                exact, kept_exact = mdl.predict(Q[c], return_kept=True)
                rel = np.max(np.abs(exact - ref[c]) / np.maximum(1, np.abs(ref[c])))
                worst = max(worst, rel)
                # the model's threshold: the same bits unless it drops a further neighbour
                mdl.tau = E.TAU
                pred, kept = mdl.predict(Q[c], return_kept=True)
                assert set(kept) <= set(kept_exact)
                if kept == kept_exact:
                    assert np.array_equal(pred, exact)
                else:
                    dropped += 1
    return worst, under, total, dropped


def test_predictions_agree_with_the_reference_where_it_is_well_conditioned():
    worst, under, total, dropped = _compare_predictions(golden('elm.npz'), WEIGHTS, MS)
    print(f'largest relative difference {worst:.3e} over {under} of {total} cases (measured {PRED_MEASURED:.3e}); '
          f'TAU = 2^-8 drops a further neighbour in {dropped} of them')
    assert under >= 0.9 * total, (under, total)   # the cap must not hide a failure
    assert worst <= PRED_BOUND, worst


@pytest.mark.parametrize('d,res,deg', WIDE_WEIGHTS)
def test_wide_weights_equal_the_reference_bitwise(d, res, deg):
    z = golden('elm_wide.npz')
    tag = f'w__{d}_{res}_{deg}'
    bias, C = E.draw_weights(d, 47, res, deg)
    assert C.shape == (res, E.n_poly(d, deg))
    assert np.array_equal(bias, z[tag + '__bias'][:, 0]) and np.array_equal(C, z[tag + '__C'])


def test_wide_predictions_agree_with_the_reference_where_it_is_well_conditioned():
    """The restatement at the reference's default width (res_size = 500) and at degree 1 with m up to 16:
    every dot product over res_size longer than a wave, 40 training rows."""
    z = golden('elm_wide.npz')
    assert z['w__3_500_2__X'].shape == (10, 40, 3) and z['w__16_200_1__pred_m16'].shape == (10, 16)
    worst, under, total, dropped = _compare_predictions(z, WIDE_WEIGHTS, WIDE_MS)
    print(f'wide: largest relative difference {worst:.3e} over {under} of {total} cases (measured '
          f'{WIDE_MEASURED:.3e}); TAU = 2^-8 drops a further neighbour in {dropped} of them')
    assert total == 90 and under >= 0.9 * total, (under, total)   # the cap must not hide a failure
    assert worst <= WIDE_BOUND, worst


@pytest.mark.parametrize('name', sorted(RUNS))
def test_loop_first_correction_agrees_with_the_reference(name):
    z = golden('elm.npz')
    r = cpu_loop(name, E.TAU_EXACT)
    ref = z[f'run__{name}__elm__u']
    assert np.max(np.abs(r['u'][:, :, 0] - ref[:, :, 0])) < 1e-13   # the initial coarse sweep
    rel = np.max(np.abs(r['u'][:, :, 1] - ref[:, :, 1]) / np.maximum(1, np.abs(ref[:, :, 1])))
    print(f'{name}: column 1 differs by {rel:.3e} (measured {COL1[name][0]:.3e})')
    assert rel <= COL1[name][1], rel


@pytest.mark.parametrize('name', sorted(RUNS))
def test_loop_converges_no_later_than_classic_parareal(name):
    """The convergence condition, first half, with TAU = 2^-8: K = 19 (Lorenz; classic
    21, the reference's ELM 19) and K = 7 (FHN-ODE; classic 11, the reference's ELM 7)."""
    z = golden('elm.npz')
    r = cpu_loop(name)
    print(f"{name}: K = {r['k']}, classic {int(z[f'run__{name}__parareal__k'])}, reference ELM "
          f"{int(z[f'run__{name}__elm__k'])}")
    assert r['converged'] and r['k'] <= int(z[f'run__{name}__parareal__k'])


@pytest.mark.parametrize('name', sorted(RUNS))
def test_loop_final_state_is_within_10_eps_of_the_serial_fine_solution(name):
    """The convergence condition, second half: max |u_final - fine| <= 10 eps = 5e-6 at
    the slice boundaries, for the last returned column.  It decides the threshold: from 2^-52 in
    factors of 2^4, Lorenz is 2.0e-4 .. 4.0e-4 (K = 18 or 19) at every value up to 2^-12 and 4.64e-6
    (K = 19) at 2^-8, the first value that meets it; FHN-ODE is 3.3e-9 (K = 7) at 2^-52 and
    4.49e-9 (K = 7) at 2^-8.  Lorenz's margin is thin and not monotone in the threshold (4.28e-5 at
    2^-4): the convergence test bounds the increment between iterates, not the distance to the fine
    solution, which on this chaotic run is 7.46e-3 for classic Parareal and 5.8e-5 for the
    reference's own ELM run."""
    r = cpu_loop(name)
    e = np.max(np.abs(r['u'][:, :, -1] - serial_fine(name)))
    print(f'{name}: final state is {e:.3e} from the serial fine solution (10 eps = {10 * EPS:.1e})')
    assert e <= 10 * EPS, e


def test_duplicated_and_collinear_neighbours_are_dropped():
    rng = np.random.default_rng(5)
    res, d = 20, 3
    H = rng.integers(-8, 9, (4, res)).astype(float)
    Y = rng.uniform(-1, 1, (4, d))
    hq = rng.uniform(-1, 1, res)
    base = E.solve(H, Y, hq)
    # a duplicate of the nearest row, and of a later one: z = 0, resp. r = 0 after the projection
    for at, src in ((1, 0), (2, 1), (4, 2)):
        Hd, Yd = np.insert(H, at, H[src], 0), np.insert(Y, at, Y[src], 0)
        p, kept = E.solve(Hd, Yd, hq, return_kept=True)
        assert at not in kept and np.all(np.isfinite(p))
        assert np.array_equal(p, base)
    # exactly collinear: h_c = h_0 + 2 (h_1 - h_0), exact in fp64 on these integer rows
    hc = H[0] + 2 * (H[1] - H[0])
    Hc, Yc = np.insert(H, 2, hc, 0), np.insert(Y, 2, rng.uniform(-1, 1, d), 0)
    p, kept = E.solve(Hc, Yc, hq, return_kept=True)
    assert kept == [1, 3, 4] and np.all(np.isfinite(p)) and np.array_equal(p, base)
    # one neighbour: its target
    assert np.array_equal(E.solve(H[:1], Y[:1], hq), Y[0])
    # through the model, with a training set that holds the same state twice (Parareal's do)
    X = rng.uniform(-1, 1, (6, d))
    Yx = rng.uniform(-1, 1, (6, d))
    q = X[2] + 1e-3
    a = E.ElmRef(d, m=3)
    a.fit(np.vstack([X, X[2:3]]), np.vstack([Yx, Yx[2:3]]))
    b = E.ElmRef(d, m=2)
    b.fit(X, Yx)
    assert np.array_equal(a.predict(q), b.predict(q))


def test_hidden_rows_do_not_depend_on_their_batch():
    rng = np.random.default_rng(6)
    for d, res, deg in ((3, 20, 2), (50, 7, 2)):   # n_poly 10 and 1326 (two chunks)
        bias, C = E.draw_weights(d, 47, res, deg)
        X = rng.uniform(-1, 1, (5, d))
        H = E.hidden(X, bias, C, deg)
        assert np.array_equal(H, np.vstack([E.hidden(X[:2], bias, C, deg), E.hidden(X[2:], bias, C, deg)]))
        ref = np.maximum(0, bias[:, None] + C @ np.array([E.features(x, deg) for x in X]).T).T
        assert np.max(np.abs(H - ref)) < 1e-12 and np.any(H == 0) and np.any(H > 0)


# ------------------------------------------------------------------------------------- the surface
def test_unsupported_settings_raise_without_a_gpu(monkeypatch):
    import nngp_amd
    from nngp_amd import models
    for loss in ('tanh', 'radbad'):
        with pytest.raises(NotImplementedError, match='relu'):
            nngp_amd.ELM(d=3, N=8, loss=loss)
        with pytest.raises(NotImplementedError, match='relu'):
            nngp_amd.ELM_base(d=3, loss=loss)
    with pytest.raises(NotImplementedError, match='degree 1 or 2'):
        nngp_amd.ELM(d=3, N=8, degree=3)
    with pytest.raises(NotImplementedError, match='alpha == 0'):
        nngp_amd.ELM(d=3, N=8, alpha=0.1)
    for kw in (dict(m=0), dict(m=17), dict(res_size=0), dict(res_size=1025)):
        with pytest.raises(ValueError, match='supported'):
            nngp_amd.ELM(d=3, N=8, **kw)
    # a C that cannot fit the device: refused with the sizes before anything is drawn
    with pytest.raises(ValueError, match=r'1024 x 32012001 doubles = 262242312192 bytes'):
        nngp_amd.ELM(d=8000, N=8, res_size=1024)
    mdl = nngp_amd.ELM(d=3, N=8)
    assert mdl.name == 'ELM' and mdl.ELM.bias.shape == (20, 1) and mdl.ELM.C.shape == (20, 10) and mdl.ELM.m == 4
    base = nngp_amd.ELM_base(d=3)
    assert base.C.shape == (500, 10) and base.m == 5 and models.elm_n_poly(800, 2) == 321201
    bias, C = E.draw_weights(3, 47, 20, 2)
    assert np.array_equal(mdl.ELM.bias[:, 0], bias) and np.array_equal(mdl.ELM.C, C)
    # the driver: refusals come before any GPU work
    ode = nngp_amd.Lorenz(normalization='-11')
    s = nngp_amd.SolverRK(ode.get_vector_field(), Ng=6, Nf=45, F='RK4', G='RK4')
    p = nngp_amd.Parareal(ode, s, [0, 18], 4, verbose=None)
    with pytest.raises(NotImplementedError, match='relu'):
        p.run(model='elm', loss='tanh')
    with pytest.raises(Exception, match='Not implemented'):
        nngp_amd.legacy.Parareal(ode_name='lorenz_n', epsilon=5e-7, verbose=None).run(model='elm')
    import torch.distributed as dist
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)
    with pytest.raises(NotImplementedError, match='one rank'):
        p.run(model='elm')


def test_argument_errors_come_back_without_a_hip_call():
    import nngp_amd
    L = nngp_amd.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: validation fails first
    assert L.nngp_elm_hidden(one, 4, 3, 3, 20, one, one, one, None) == -1
    assert b'degree' in L.nngp_last_error()
    assert L.nngp_elm_hidden(one, 4, 3, 2, 1025, one, one, one, None) == -1
    assert b'res_size' in L.nngp_last_error()
    assert L.nngp_elm_hidden(one, 4, 0, 2, 20, one, one, one, None) == -1
    assert L.nngp_elm_hidden(one, -1, 3, 2, 20, one, one, one, None) == -1
    assert L.nngp_elm_hidden(None, 4, 3, 2, 20, one, one, one, None) == -1
    assert L.nngp_elm_hidden(one, 4, 3, 2, 20, None, one, one, None) == -1
    assert L.nngp_elm_hidden(None, 0, 3, 2, 20, one, one, None, None) == 0   # no rows: nothing to do
    pred = lambda rows, m, x=one: L.nngp_elm_predict(x, one, one, rows, 3, one, m, 2, 20, one, one, one, None, None,
                                                     None)
    assert pred(10, 17) == -1 and b'm' in L.nngp_last_error()
    assert pred(3, 4) == -1
    assert pred(10, 0) == -1
    assert pred(10, 4, None) == -1
    assert L.nngp_elm_predict(one, one, one, 10, 3, one, 4, 2, 20, one, one, None, None, None, None) == -1
    cs = nngp_amd._lib.CSystem(0, 3, 0, 0, (ctypes.c_double * 4)(), None)
    sweep = lambda I, N, m, rows=10, sys=ctypes.byref(cs): L.nngp_elm_sweep(
        sys, 4, 0, 6, one, I, N, one, one, one, one, one, rows, m, 2, 20, one, one, None, None)
    assert sweep(3, 2, 4) == -1
    assert sweep(0, 4, 17) == -1
    assert sweep(0, 4, 4, rows=2) == -1
    assert sweep(0, 4, 4, sys=None) == -1
