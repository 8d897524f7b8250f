"""DiffReact without a GPU: the Python surface against the reference's recorded constructor
outputs (tests/golden/diffreact.npz, written by gen_diffreact.py from the reference itself), the
library's shape refusals (made before any HIP call), and the NumPy yardstick that
tests/test_gpu_diffreact.py compares the kernels with bit for bit -- the RK stepper against the
CPU oracle on Lorenz, the right-hand side against the reference's."""
import ctypes

import numpy as np
import pytest

import oracle as O
from conftest import golden
from diffreact_ref import DiffReactNP, lorenz_np, rk_np


def test_diffreact_is_exported():
    import nngp_amd
    assert hasattr(nngp_amd, 'DiffReact')
    assert 'DiffReact' in nngp_amd.__all__
    from nngp_amd import _lib
    assert _lib.SYS_DIFFREACT == 9


@pytest.mark.parametrize('d_x', [4, 10])
@pytest.mark.parametrize('norm', [None, '-11'])
def test_constructor_equals_reference(d_x, norm):
    import nngp_amd
    R = golden('diffreact.npz')
    tag = f'init__{d_x}{"_n" if norm else ""}'
    ode = nngp_amd.DiffReact(d_x=d_x, normalization=norm) if norm else nngp_amd.DiffReact(d_x=d_x)
    d = 2 * d_x * d_x
    assert np.array_equal(ode.get_init_cond(), R[tag + '__u0'])
    assert ode.name == str(R[tag + '__name']) == f'DiffReact2D_{d_x}'
    assert ode.get_dim() == int(R[tag + '__dim']) == d
    assert np.array_equal(np.asarray(ode.normalizer.mn, dtype=float), R[tag + '__mn'])
    assert np.array_equal(np.asarray(ode.normalizer.mx, dtype=float), R[tag + '__mx'])
    assert (ode.d_x, ode.d_y, ode.d, ode.Du, ode.Dv, ode.k) == (d_x, d_x, d, 1e-3, 5e-3, 5e-3)
    assert ode.kind == 9 and ode.nx == d_x and ode.param == (1e-3, 5e-3, 5e-3)
    assert ode.normalized == (norm == '-11')


def test_constructor_arguments_reach_the_descriptor():
    import nngp_amd
    ode = nngp_amd.DiffReact(d_x=5, Du=2e-3, Dv=1e-2, k=1e-3, seed=7)
    assert ode.param == (2e-3, 1e-2, 1e-3) and ode.nx == 5 and ode.d == 50
    assert np.array_equal(ode.get_init_cond(), np.random.default_rng(7).uniform(size=50))


@pytest.mark.parametrize('nx,d,word', [(33, 2 * 33 * 33, '32'), (2, 8, '3 <= nx'), (10, 199, '2 nx^2'),
                                       (10, 202, '2 nx^2')])
def test_library_refuses_unsupported_shapes_without_a_gpu(nx, d, word):
    """nx outside 3..32 or d != 2 nx^2: NNGP_E_ARG from field_args, before any HIP call (the
    pointers are placeholders that are never dereferenced)."""
    from nngp_amd import _lib
    L = _lib.lib()
    p = (ctypes.c_double * 4)(1e-3, 5e-3, 5e-3, 0.0)
    cs = _lib.CSystem(_lib.SYS_DIFFREACT, d, nx, 0, p, None)
    buf = (ctypes.c_double * 8)()
    ptr = ctypes.addressof(buf)
    for tab in (1, 2, 4, 8):
        for mode in (_lib.STEP_FIXED, _lib.STEP_LINSPACE, _lib.STEP_FIXED | _lib.STEP_CONTRACT):
            assert L.nngp_rk_batch(ctypes.byref(cs), tab, mode, 1, ptr, ptr, 3, ptr, ptr, None) == -1
            msg = L.nngp_last_error().decode()
            assert 'DiffReact' in msg and word in msg, msg
    assert L.nngp_rhs_batch(ctypes.byref(cs), 1, ptr, ptr, None) == -1
    assert 'DiffReact' in L.nngp_last_error().decode()


def test_python_square_is_the_product():
    """The library forms dx**2 as dx*dx; the reference's Python `d_x**2` gives the same double at
    every supported grid, so its host-side coefficients are the reference's bit for bit."""
    for nx in range(3, 33):
        dx = (1.0 - (-1.0)) / nx
        assert dx**2 == dx * dx


@pytest.mark.parametrize('order', [1, 4])
@pytest.mark.parametrize('mode', ['fixed', 'linspace'])
def test_numpy_stepper_is_bitwise_the_oracle_on_lorenz(order, mode):
    so = O.System('lorenz', normalized=False)
    rng = np.random.default_rng(order)
    m = O.STEP_FIXED if mode == 'fixed' else O.STEP_LINSPACE
    for steps, t0, t1 in [(7, 0.3, 0.41), (1, 0.0, 0.01), (12, 1.7, 1.9)]:
        u0 = np.array([-15.0, -15.0, 20.0]) + rng.standard_normal(3)
        got = rk_np(lorenz_np, order, t0, t1, steps, u0, mode)
        assert np.array_equal(got, so.rk(order, t0, t1, steps, u0, m)), (steps, t0, t1)
        assert np.array_equal(lorenz_np(u0), so.rhs(u0))


@pytest.mark.parametrize('key,nx,norm', [('4', 4, False), ('4_n', 4, True), ('10', 10, False), ('10_n', 10, True),
                                         ('16', 16, False), ('17', 17, False)])
def test_numpy_rhs_equals_reference(key, nx, norm):
    R = golden('diffreact.npz')
    U, ref = R[f'rhs__{key}__u'], R[f'rhs__{key}__f']
    assert not np.any(U == 0.0)   # the contract leaves the sign of an exact zero open
    f = DiffReactNP(nx, normalized=norm)
    got = np.array([f(u) for u in U])
    assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))


@pytest.mark.parametrize('key,nx,norm', [('4', 4, False), ('10_n', 10, True), ('17', 17, False)])
@pytest.mark.parametrize('order', [1, 4])
def test_numpy_stepper_equals_reference_rk(key, nx, norm, order):
    R = golden('diffreact.npz')
    k = f'rk__{key}__RK{order}'
    t0, t1, steps = R[k + '__span']
    f = DiffReactNP(nx, normalized=norm)
    for mode in ('fixed', 'linspace'):
        ref = R[k + '__' + mode]
        got = rk_np(f, order, t0, t1, int(steps), R[k + '__u0'], mode)
        assert np.max(np.abs(got - ref)) <= 1e-13 * max(1.0, np.max(np.abs(ref)))
