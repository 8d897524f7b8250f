"""PolyODE without a GPU: the NumPy yardstick of tests/test_gpu_poly.py (tests/poly_ref.py) against
the CPU oracle -- Brusselator written as monomials is bit for bit the oracle's built-in one, and the
stepper with all four tableaux is the oracle's on Lorenz -- and against the reference's recorded
outputs (tests/golden/poly.npz, written by gen_poly.py from two subclasses of the reference's ODE);
the library's refusals, every one made before any HIP call; the table handles; the Python surface."""
import ctypes

import numpy as np
import pytest

import oracle as O
from conftest import golden
from diffreact_ref import lorenz_np
from poly_ref import BRUS, LORENZ, VDP, PolyNP, lorenz96, rk_np

ORDERS = [1, 2, 4, 8]
SPANS = [(7, 0.3, 0.41), (1, 0.0, 0.01), (12, 1.7, 1.9)]
BRUS_MN, BRUS_MX = np.array([0.4, 0.9]), np.array([4.0, 5.0])


# ------------------------------------------------------------------------------------------------
# the yardstick
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm', [False, True])
def test_brusselator_rows_are_bitwise_the_oracle_rhs(norm):
    so = O.System('brus', normalized=norm)
    f = PolyNP(BRUS, BRUS_MN, BRUS_MX) if norm else PolyNP(BRUS)
    rng = np.random.default_rng(3)
    U = rng.uniform(-0.9, 0.9, (2000, 2)) if norm else np.array([1.0, 3.07]) + rng.standard_normal((2000, 2))
    ref = np.array([so.rhs(u) for u in U])
    assert np.array_equal(f(U), ref)              # batched
    assert np.array_equal(f(U[5]), ref[5])        # one state


@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('mode', ['fixed', 'linspace'])
def test_brusselator_rows_are_bitwise_the_oracle_rk(norm, order, mode):
    so = O.System('brus', normalized=norm)
    f = PolyNP(BRUS, BRUS_MN, BRUS_MX) if norm else PolyNP(BRUS)
    m = O.STEP_FIXED if mode == 'fixed' else O.STEP_LINSPACE
    rng = np.random.default_rng(order)
    for steps, t0, t1 in SPANS:
        u0 = rng.uniform(-0.5, 0.5, 2) if norm else np.array([1.0, 3.07]) + 0.1 * rng.standard_normal(2)
        assert np.array_equal(rk_np(f, order, t0, t1, steps, u0, mode), so.rk(order, t0, t1, steps, u0, m)), steps


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('mode', ['fixed', 'linspace'])
def test_stepper_is_bitwise_the_oracle_on_lorenz(order, mode):
    """the built-in Lorenz expressions (Lorenz as monomials rounds once more: 10*u1 - 10*u0)"""
    so = O.System('lorenz', normalized=False)
    rng = np.random.default_rng(order)
    m = O.STEP_FIXED if mode == 'fixed' else O.STEP_LINSPACE
    for steps, t0, t1 in SPANS:
        u0 = np.array([-15.0, -15.0, 20.0]) + rng.standard_normal(3)
        assert np.array_equal(rk_np(lorenz_np, order, t0, t1, steps, u0, mode), so.rk(order, t0, t1, steps, u0, m))


def test_batched_stepper_is_the_single_slice_stepper():
    f = PolyNP(LORENZ)
    rng = np.random.default_rng(0)
    U0 = np.array([-15.0, -15.0, 20.0]) + rng.standard_normal((5, 3))
    T0 = 0.1 * np.arange(5)
    T1 = T0 + 0.05 + 0.01 * np.arange(5)
    for mode in ('fixed', 'linspace'):
        got = rk_np(f, 8, T0, T1, 7, U0, mode)
        assert np.array_equal(got, np.array([rk_np(f, 8, T0[i], T1[i], 7, U0[i], mode) for i in range(5)]))


def test_lorenz_rows_stay_within_rounding_of_the_oracle():
    so = O.System('lorenz', normalized=False)
    rng = np.random.default_rng(1)
    U = np.array([-15.0, -15.0, 20.0]) + rng.standard_normal((500, 3))
    ref = np.array([so.rhs(u) for u in U])
    assert np.max(np.abs(PolyNP(LORENZ)(U) - ref) / np.maximum(1, np.abs(ref))) <= 1e-13


def test_rows_without_terms_and_constant_rows():
    f = PolyNP([[], [(0.7, ())], [(-0.3, (2,)), (0.5, (0, 1))]])
    out = f(np.array([2.0, -3.0, 5.0]))
    assert out[0] == 0.0 and not np.signbit(out[0]) and out[1] == 0.7 and out[2] == -0.3 * 5.0 + (0.5 * 2.0) * -3.0


def _rows(key):
    return VDP if key.startswith('vdp') else lorenz96(40)


def _bounds(key):
    return (np.array([-2.5, -3.0]), np.array([2.5, 3.0])) if key.startswith('vdp') else (-12.0, 16.0)


@pytest.mark.parametrize('key', ['vdp', 'vdp_n', 'l96', 'l96_n'])
def test_rhs_against_the_reference(key):
    R = golden('poly.npz')
    U, ref = R[f'rhs__{key}__u'], R[f'rhs__{key}__f']
    f = PolyNP(_rows(key), *_bounds(key)) if key.endswith('_n') else PolyNP(_rows(key))
    got = f(U)
    assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))
    if not key.endswith('_n'):
        assert np.array_equal(got, ref)   # the reference's _f_np is written in the contract's order


@pytest.mark.parametrize('key', ['vdp', 'vdp_n', 'l96', 'l96_n'])
@pytest.mark.parametrize('order', ORDERS)
def test_rk_against_the_reference(key, order):
    R = golden('poly.npz')
    k = f'rk__{key}__RK{order}'
    t0, t1, steps = R[k + '__span']
    f = PolyNP(_rows(key), *_bounds(key)) if key.endswith('_n') else PolyNP(_rows(key))
    for mode in ('fixed', 'linspace'):
        ref = R[k + '__' + mode]
        got = rk_np(f, order, t0, t1, int(steps), R[k + '__u0'], mode)
        assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))


def test_recorded_parareal_runs_are_not_decided_by_chaos():
    """gen_poly.py repeated each classic run from u0 + 1e-13: K and conv_int stayed and u moved by
    less than 1e-10, so the GPU test's 1e-9 bound measures arithmetic, not sensitivity"""
    R = golden('poly.npz')
    for key in ('vdp', 'l96'):
        shift, moved, same = R[f'para__{key}__perturbed']
        assert shift == 1e-13 and same == 1.0 and moved < 1e-10


# ------------------------------------------------------------------------------------------------
# the library: tables, handles, refusals (no HIP call is reached)
# ------------------------------------------------------------------------------------------------
def _create(L, d, row_ptr, coef, idx):
    rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
    cf = np.ascontiguousarray(coef, dtype=np.float64)
    ix = np.ascontiguousarray(idx, dtype=np.int16).reshape(-1)
    h = ctypes.c_int32(0)
    rc = L.nngp_poly_create(d, len(cf), rp.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                            cf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                            ix.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), ctypes.byref(h))
    return rc, h.value


GOOD = dict(d=2, row_ptr=[0, 1, 2], coef=[1.0, -2.0], idx=[[0, 1, -1], [1, -1, -1]])


@pytest.mark.parametrize('change,word', [
    (dict(d=0), 'd=0'), (dict(d=2049), 'd=2049'),
    (dict(row_ptr=[1, 1, 2]), 'row_ptr[0]'), (dict(row_ptr=[0, 2, 1]), 'non-decreasing'),
    (dict(row_ptr=[0, 1, 1]), 'row_ptr[d]'), (dict(row_ptr=[0, 1, 3]), 'n_terms'),
    (dict(idx=[[0, 2, -1], [1, -1, -1]]), 'index 2'), (dict(idx=[[0, -2, -1], [1, -1, -1]]), 'index -2'),
    (dict(idx=[[-1, 0, -1], [1, -1, -1]]), 'after a -1'),
    (dict(coef=[np.inf, 1.0]), 'finite'), (dict(coef=[1.0, np.nan]), 'finite'),
])
def test_create_refuses_a_bad_table(change, word):
    from nngp_amd import _lib
    L = _lib.lib()
    rc, h = _create(L, **dict(GOOD, **change))
    msg = L.nngp_last_error().decode()
    assert rc == -1 and h == 0 and 'poly' in msg and word in msg, msg


def test_create_refuses_too_many_terms_and_null_arguments():
    from nngp_amd import _lib
    L = _lib.lib()
    h = ctypes.c_int32(0)
    rp = (ctypes.c_int32 * 3)(0, 1, 2)
    assert L.nngp_poly_create(2, 1048577, rp, None, None, ctypes.byref(h)) == -1
    assert 'poly' in L.nngp_last_error().decode() and 'n_terms' in L.nngp_last_error().decode()
    assert L.nngp_poly_create(2, -1, rp, None, None, ctypes.byref(h)) == -1
    assert L.nngp_poly_create(2, 2, rp, None, None, ctypes.byref(h)) == -1
    assert 'poly' in L.nngp_last_error().decode()
    assert L.nngp_poly_create(2, 0, None, None, None, ctypes.byref(h)) == -1
    assert L.nngp_poly_create(2, 0, (ctypes.c_int32 * 3)(0, 0, 0), None, None, None) == -1
    assert h.value == 0


def test_handles_are_created_destroyed_and_reused():
    from nngp_amd import _lib
    L = _lib.lib()
    rc, a = _create(L, **GOOD)
    rc2, b = _create(L, **GOOD)
    assert rc == 0 and rc2 == 0 and a >= 1 and b >= 1 and a != b
    rc, empty = _create(L, d=3, row_ptr=[0, 0, 0, 0], coef=[], idx=[])   # a table without terms is valid
    assert rc == 0 and empty not in (a, b)
    assert L.nngp_poly_destroy(a) == 0
    assert L.nngp_poly_destroy(a) == -1 and 'poly' in L.nngp_last_error().decode()   # twice
    rc, c = _create(L, **GOOD)
    assert rc == 0 and c == a                        # the freed slot is handed out again
    for h in (b, c, empty):
        assert L.nngp_poly_destroy(h) == 0
    for h in (0, -1, 10 ** 6):
        assert L.nngp_poly_destroy(h) == -1


@pytest.mark.parametrize('case', ['unknown', 'destroyed', 'zero', 'other_d'])
def test_library_refuses_bad_descriptors_without_a_gpu(case):
    """NNGP_E_ARG from the host-side lookup, before any HIP call (the pointers are placeholders that
    are never dereferenced): every tableau and step mode, the trajectory and the right-hand side."""
    from nngp_amd import _lib
    L = _lib.lib()
    rc, live = _create(L, **GOOD)
    assert rc == 0
    try:
        d, word = 2, 'handle'
        if case == 'unknown':
            h = live + 1000
        elif case == 'zero':
            h = 0
        elif case == 'destroyed':
            rc, h = _create(L, **GOOD)
            assert L.nngp_poly_destroy(h) == 0
        else:
            h, d, word = live, 3, 'd=3'
        cs = _lib.CSystem(_lib.SYS_POLY, d, h, 0, (ctypes.c_double * 4)(), None)
        buf = (ctypes.c_double * 16)()
        ptr = ctypes.addressof(buf)
        for tab in (1, 2, 4, 8):
            for mode in (_lib.STEP_FIXED, _lib.STEP_LINSPACE, _lib.STEP_FIXED | _lib.STEP_CONTRACT,
                         _lib.STEP_LINSPACE | _lib.STEP_CONTRACT):
                assert L.nngp_rk_batch(ctypes.byref(cs), tab, mode, 1, ptr, ptr, 3, ptr, ptr, None) == -1
                msg = L.nngp_last_error().decode()
                assert 'poly' in msg and word in msg, msg
                assert L.nngp_rk_traj(ctypes.byref(cs), tab, mode, 1, ptr, ptr, 3, 1, ptr, ptr + 64, None) == -1
                assert 'poly' in L.nngp_last_error().decode()
            assert L.nngp_rk_batch_grid(ctypes.byref(cs), tab, 1, ptr, ptr, 3, ptr, 3, ptr, ptr, None) == -1
            assert 'poly' in L.nngp_last_error().decode()
        assert L.nngp_rhs_batch(ctypes.byref(cs), 1, ptr, ptr, None) == -1
        msg = L.nngp_last_error().decode()
        assert 'poly' in msg and word in msg, msg
    finally:
        L.nngp_poly_destroy(live)


# ------------------------------------------------------------------------------------------------
# the Python surface
# ------------------------------------------------------------------------------------------------
def test_polyode_is_exported():
    import nngp_amd
    from nngp_amd import _lib
    assert 'PolyODE' in nngp_amd.__all__ and issubclass(nngp_amd.PolyODE, nngp_amd.ODE)
    assert _lib.SYS_POLY == 10 and nngp_amd.PolyODE.kind == 10


def test_polyode_descriptor_fields():
    import nngp_amd
    from nngp_amd import _lib
    ode = nngp_amd.PolyODE(BRUS, [1, 3.07])
    assert ode.name == 'PolyODE' and ode.d == 2 and ode.get_dim() == 2 and not ode.normalized and ode.param == ()
    assert ode._handle is None                      # made on first use of the descriptor
    f = ode.get_vector_field()
    assert isinstance(f, nngp_amd.VectorField) and ode._handle is None
    cs = f.csystem('cpu')
    assert (cs.kind, cs.d, cs.normalized, cs.norm) == (10, 2, 0, None) and cs.nx == ode._handle >= 1
    assert ode.get_vector_field().csystem('cpu').nx == cs.nx       # one table per object
    assert np.array_equal(ode.get_init_cond(), [1.0, 3.07])
    h = ode._handle
    ode.destroy()
    assert _lib.lib().nngp_poly_destroy(h) == -1     # gone
    other = nngp_amd.PolyODE(LORENZ, [-15, -15, 20], name='Lorenz as monomials')
    assert other.nx == h and other.name == 'Lorenz as monomials'   # the slot is reused
    del other
    assert _lib.lib().nngp_poly_destroy(h) == -1     # destroyed with the object


def test_polyode_normalisation_needs_bounds():
    import nngp_amd
    with pytest.raises(ValueError, match='mn and mx'):
        nngp_amd.PolyODE(BRUS, [1, 3.07], normalization='-11')
    ode = nngp_amd.PolyODE(BRUS, [1, 3.07], mn=BRUS_MN, mx=BRUS_MX, normalization='-11')
    ref = nngp_amd.Brusselator(normalization='-11')
    assert ode.normalized and np.array_equal(ode.get_init_cond(), ref.get_init_cond())
    assert np.array_equal(ode.normalizer.device_table(2), ref.normalizer.device_table(2))


@pytest.mark.parametrize('terms,u0,word', [
    ([[(1.0, (0,))]], [1.0, 2.0], 'rows'), ([[(1.0, (0, 0, 0, 0))]], [1.0], 'degree'),
    ([[(1.0, (1,))]], [1.0], 'index'), ([[(1.0, (-1,))]], [1.0], 'index'), ([[(np.nan, ())]], [1.0], 'finite'),
    ([[]] * 2049, np.ones(2049), '2048'),
])
def test_polyode_refuses_bad_terms(terms, u0, word):
    import nngp_amd
    with pytest.raises(ValueError, match=word):
        nngp_amd.PolyODE(terms, u0)


def test_solvers_accept_a_polyode_unchanged():
    import nngp_amd
    ode = nngp_amd.PolyODE(VDP, [2.0, 0.0], mn=[-2.5, -3.0], mx=[2.5, 3.0], normalization='-11')
    s = nngp_amd.SolverRK(ode.get_vector_field(), Ng=4, Nf=40, F='RK4', G='RK1')
    p = nngp_amd.Parareal(ode, s, [0, 8], 16, verbose=None)
    assert p.N == 16 and s.step_mode == 0
    assert nngp_amd.SolverRK(ode.get_vector_field(), 4, 40, 'RK8', 'RK2', step_mode='linspace', fma=True).step_mode == 17
