"""Burgers away from d = 128: the GPU right-hand side and propagator against the reference's own
outputs at d = 3 .. 300 (tests/golden/burgers_sizes.npz), and short nnGParareal runs whose coarse
propagator is the in-kernel Burgers G (csrc/nngp_gp.hip chain_burgers_g: gdist_kernel, the default
head of every sweep slice; guess_chain_kernel; the NNGP_CHAIN=1 chain) at 1, 2, 3 and 4 elements
per lane, every tableau, both step modes and both normalisations, against the oracle's Parareal
loop bit for bit.

The sweeps: N = 16 slices of [0, 0.625], F = RK4 with 400 steps per slice, nn = 12, seed 45, three
iterations; epsilon = 1e-13 keeps every sweep at full length (on the oracle each row gives
conv_int == [1, 2, 3] with every iterate finite -- asserted on the oracle's run, not on the code
under test).  The RK8 row takes Ng = 8: at Ng = 4 the oracle's initial coarse solve is not finite,
at Ng = 16 it converges a slice early."""
import numpy as np
import pytest

import oracle as O
from conftest import golden
from systems_table import burgers_u0, oracle_burgers, product_burgers

pytestmark = pytest.mark.gpu


def _t(torch, a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------
# against the reference's recorded outputs
# ------------------------------------------------------------------------------------------------
SIZES = [3, 5, 64, 65, 192, 256, 300]
CASES = [(d, norm) for d in SIZES for norm in (False, True)]
IDS = [f'{d}{"_n" if norm else ""}' for d, norm in CASES]


@pytest.mark.parametrize('d,norm', CASES, ids=IDS)
def test_rhs_within_tolerance_of_reference(gpu, d, norm):
    R = golden('burgers_sizes.npz')
    tag = f'{d}{"_n" if norm else ""}'
    ref = R[f'rhs__{tag}__f']
    got = product_burgers(gpu, d, norm).get_vector_field()(0.0, R[f'rhs__{tag}__u'])
    assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))


@pytest.mark.parametrize('mode', ['fixed', 'linspace'])
@pytest.mark.parametrize('tab', ['RK1', 'RK4', 'RK8'])
@pytest.mark.parametrize('d,norm', CASES, ids=IDS)
def test_rk_within_tolerance_of_reference(gpu, d, norm, tab, mode):
    import torch
    R = golden('burgers_sizes.npz')
    k = f'rk__{d}{"_n" if norm else ""}__{tab}'
    t0, t1, steps = R[k + '__span']
    s = gpu.SolverRK(product_burgers(gpu, d, norm).get_vector_field(), Ng=int(steps), Nf=int(steps), F=tab, G=tab,
                     step_mode=mode)
    got = s.run_F_batch(_t(torch, [t0]), _t(torch, [t1]), _t(torch, R[k + '__u0'][None, :])).cpu().numpy()[0]
    ref = R[k + '__' + mode]
    assert np.max(np.abs(got - ref)) <= 1e-13 * max(1.0, np.max(np.abs(ref)))


# ------------------------------------------------------------------------------------------------
# sweeps with the in-kernel G
# ------------------------------------------------------------------------------------------------
# id -> (d, normalised, G, Ng, step mode)
ROWS = {
    'd64_identity_RK2': (64, False, 'RK2', 8, 'fixed'),
    'd192_norm11_RK1_linspace': (192, True, 'RK1', 16, 'linspace'),
    'd256_norm11_RK4': (256, True, 'RK4', 16, 'fixed'),
    'd128_identity_RK1': (128, False, 'RK1', 8, 'fixed'),
    'd256_identity_RK8_linspace': (256, False, 'RK8', 8, 'linspace'),
}
TSPAN, N, NF = [0, 0.625], 16, 400
RUN = dict(model='nngp', nn=12, seed=45, early_stop=3)


def _same(a, b):
    a, b = np.nan_to_num(a, nan=7.0), np.nan_to_num(b, nan=7.0)   # columns not written stay NaN
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope='module')
def sweeps(gpu):
    """row -> (oracle loop's result, the default GPU run): computed once, shared, left unchanged"""
    cache = {}

    def get(row):
        if row not in cache:
            d, norm, G, Ng, mode = ROWS[row]
            so = oracle_burgers(d, norm)
            o = O.parareal(so, TSPAN, N, Ng, NF, G, 'RK4', epsilon=1e-13, model='nngp', nn=12, seed=45,
                           u0=so.fit(burgers_u0(d)), early_stop=3,
                           step_mode=O.STEP_FIXED if mode == 'fixed' else O.STEP_LINSPACE)
            # the condition on the inputs: three full sweeps, all finite -- on the oracle
            assert o['conv_int'] == [1, 2, 3] and o['k'] == 3 and np.all(np.isfinite(o['u']))
            r = _gpu_run(gpu, row)
            for a in (o['u'], r['u']):
                a.setflags(write=False)
            cache[row] = (o, r)
        return cache[row]
    return get


def _gpu_run(gpu, row):
    d, norm, G, Ng, mode = ROWS[row]
    ode = product_burgers(gpu, d, norm)
    s = gpu.SolverRK(ode.get_vector_field(), Ng=Ng, Nf=NF, F='RK4', G=G, step_mode=mode)
    return gpu.Parareal(ode, s, TSPAN, N, epsilon=1e-13, verbose=None).run(**RUN)


@pytest.mark.parametrize('row', list(ROWS))
def test_sweep_is_bitwise_the_oracle_loop(gpu, sweeps, row, monkeypatch):
    for k in ('NNGP_GDIST', 'NNGP_GUESS_FUSED', 'NNGP_CHAIN'):
        monkeypatch.delenv(k, raising=False)
    o, r = sweeps(row)
    print(row, 'K', r['k'], 'conv_int', r['conv_int'], 'spec hits', r['timings']['spec_hits'])
    assert r['k'] == o['k'] and list(r['conv_int']) == o['conv_int']
    assert _same(r['u'], o['u'])


@pytest.mark.parametrize('row', list(ROWS))
def test_sweep_without_the_fused_heads_is_bitwise(gpu, sweeps, row, monkeypatch):
    """G and the distances as separate launches (NNGP_GDIST=0) and the guesses by the launch loop
    (NNGP_GUESS_FUSED=0): the G launch's wave kernel in place of chain_burgers_g"""
    for k in ('NNGP_GDIST', 'NNGP_GUESS_FUSED', 'NNGP_CHAIN'):
        monkeypatch.delenv(k, raising=False)
    _, r = sweeps(row)
    monkeypatch.setenv('NNGP_GDIST', '0')
    monkeypatch.setenv('NNGP_GUESS_FUSED', '0')
    b = _gpu_run(gpu, row)
    assert b['k'] == r['k'] and list(b['conv_int']) == list(r['conv_int'])
    assert b['timings']['spec_hits'] == r['timings']['spec_hits']
    assert _same(b['u'], r['u'])


@pytest.mark.parametrize('row', list(ROWS))
def test_sweep_on_the_fused_chain_is_bitwise(gpu, sweeps, row, monkeypatch):
    from nngp_amd import _lib
    for k in ('NNGP_GDIST', 'NNGP_GUESS_FUSED', 'NNGP_CHAIN'):
        monkeypatch.delenv(k, raising=False)
    _, r = sweeps(row)
    monkeypatch.setenv('NNGP_CHAIN', '1')
    n0, _ = _lib.chain_stats()
    b = _gpu_run(gpu, row)
    print(row, 'chain launches', _lib.chain_stats()[0] - n0, 'spec hits', b['timings']['spec_hits'])
    assert b['k'] == r['k'] and list(b['conv_int']) == list(r['conv_int'])
    assert b['timings']['spec_hits'] == r['timings']['spec_hits']
    assert _same(b['u'], r['u'])
    assert _lib.chain_stats()[0] > n0
