"""The CPU oracle's Burgers (oracle/nngp_oracle.c) at the sizes the GPU matrix tests use it as the
bitwise yardstick (tests/test_gpu_rk_matrix.py), pinned to the reference's own outputs
(tests/golden/burgers_sizes.npz, written by tests/golden/gen_burgers_sizes.py): within the
project's PDE tolerances (1e-12 RHS rows -- the reference sums dense-row products in BLAS order --
and 1e-13 RK, both times max(1, max |ref|), as tests/test_gpu_kernels.py), and the oracle's
stencil form bit for bit its dense-matrix form (the reference's formulation).  No GPU."""
import numpy as np
import pytest

import oracle as O
from conftest import golden
from systems_table import burgers_h, burgers_u0, oracle_burgers

SIZES = [3, 5, 64, 65, 192, 256, 300]
CASES = [(d, norm) for d in SIZES for norm in (False, True)]
IDS = [f'{d}{"_n" if norm else ""}' for d, norm in CASES]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize('d,norm', CASES, ids=IDS)
def test_oracle_rhs_within_tolerance_of_reference(d, norm):
    R = golden('burgers_sizes.npz')
    tag = f'{d}{"_n" if norm else ""}'
    U, ref = R[f'rhs__{tag}__u'], R[f'rhs__{tag}__f']
    so = oracle_burgers(d, norm)
    # the fixture's first state is the system's initial condition
    assert np.max(np.abs(U[0] - so.fit(burgers_u0(d)))) <= 1e-15
    got = np.array([so.rhs(u) for u in U])
    assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))


@pytest.mark.parametrize('d,norm', CASES, ids=IDS)
@pytest.mark.parametrize('tab', ['RK1', 'RK4', 'RK8'])
def test_oracle_rk_within_tolerance_of_reference(d, norm, tab):
    R = golden('burgers_sizes.npz')
    k = f'rk__{d}{"_n" if norm else ""}__{tab}'
    t0, t1, steps = R[k + '__span']
    assert t1 == int(steps) * burgers_h(d)
    so = oracle_burgers(d, norm)
    for mode, m in (('fixed', O.STEP_FIXED), ('linspace', O.STEP_LINSPACE)):
        ref = R[k + '__' + mode]
        got = so.rk(int(tab[2:]), t0, t1, int(steps), R[k + '__u0'], m)
        assert np.all(np.isfinite(got))
        assert np.max(np.abs(got - ref)) <= 1e-13 * max(1.0, np.max(np.abs(ref))), mode


@pytest.mark.parametrize('d,norm', CASES, ids=IDS)
def test_oracle_stencil_is_bitwise_its_dense_form(d, norm):
    """System(dense=True) evaluates Dxx@u - u*(Dx@u) with the dense matrices, row by row in
    ascending column order; the stencil form keeps the three non-zeros in that order."""
    R = golden('burgers_sizes.npz')
    st, de = oracle_burgers(d, norm), oracle_burgers(d, norm, dense=True)
    h = burgers_h(d)
    for tab in ('RK1', 'RK4', 'RK8'):
        k = f'rk__{d}{"_n" if norm else ""}__{tab}'
        U0 = np.stack([R[k + '__u0'], R[k + '__u0'][::-1]])
        T0 = np.array([0.0, 0.375])
        for m in (O.STEP_FIXED, O.STEP_LINSPACE):
            a = st.rk_batch(int(tab[2:]), T0, T0 + 3 * h, 3, U0, m)
            b = de.rk_batch(int(tab[2:]), T0, T0 + 3 * h, 3, U0, m)
            assert np.all(np.isfinite(a)) and np.array_equal(_bits(a), _bits(b)), (tab, m)
