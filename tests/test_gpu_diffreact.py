"""DiffReact on the GPU: the element-per-thread field kernel (small grids, NNGP_RK_THREADS) and
the point-pair kernel (nx 16..32) against the NumPy restatement of the arithmetic contract
(tests/diffreact_ref.py, validated on the CPU by tests/test_diffreact_host.py) bit for bit, against
the reference's recorded outputs (tests/golden/diffreact.npz) within the project's PDE-row
tolerances, and the system-independent layers above the propagator (classic Parareal,
nnGParareal with speculation / the chain knob / the coordinate-sharded sweep, GParareal).

Grids: 3 (every point an edge or a corner), 10 (4 elements per thread), 15 (225 points, the largest
below the pair kernel's switch), 16 (256 points, exactly 4 waves), 17 (289 points, a partial last
wave with idle lanes), 32 (1024 points, the launch bound).  Inputs hold no exact zero (the
contract leaves the sign of a zero sum open; `==` ignores it)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import golden
from diffreact_ref import DiffReactNP, rk_np

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GRIDS = [3, 10, 15, 16, 17, 32]
FORCED_THREADS = '256'   # a valid element-kernel layout at every d = 2 nx^2 <= 2048 (<= 8 per thread)


def _t(torch, a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device='cuda')


def _ode(gpu, nx, norm):
    return gpu.DiffReact(d_x=nx, normalization='-11') if norm else gpu.DiffReact(d_x=nx)


def _states(nx, n, seed):
    U = np.random.default_rng(seed).uniform(-0.9, 0.9, (n, 2 * nx * nx))
    assert not np.any(U == 0.0)
    return U


def _spans(n):
    """different t0 / t1 per slice; h stays inside the explicit stability limit at nx = 32"""
    T0 = 0.25 + 0.0625 * np.arange(n)
    return T0, T0 + 0.04 + 0.003 * np.arange(n)


@pytest.mark.parametrize('nx', GRIDS)
@pytest.mark.parametrize('norm', [False, True])
def test_rhs_is_bitwise_the_contract(gpu, nx, norm):
    f = _ode(gpu, nx, norm).get_vector_field()
    U = _states(nx, 4, nx)
    ref = DiffReactNP(nx, normalized=norm)
    got = f(0.0, U)
    assert np.array_equal(got, np.array([ref(u) for u in U]))
    assert np.array_equal(f(0.0, U[1]), ref(U[1]))


@pytest.mark.parametrize('key,nx,norm', [('4', 4, False), ('4_n', 4, True), ('10', 10, False), ('10_n', 10, True),
                                         ('16', 16, False), ('17', 17, False)])
def test_rhs_within_tolerance_of_reference(gpu, key, nx, norm):
    R = golden('diffreact.npz')
    ref = R[f'rhs__{key}__f']
    got = _ode(gpu, nx, norm).get_vector_field()(0.0, R[f'rhs__{key}__u'])
    assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))


@pytest.mark.parametrize('nx', GRIDS)
@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('tab', ['RK1', 'RK4'])
@pytest.mark.parametrize('mode', ['fixed', 'linspace'])
def test_rk_is_bitwise_the_numpy_stepper(gpu, nx, norm, tab, mode):
    """7 steps (odd: a remainder step of any unrolled loop is taken), 5 slices with their own spans."""
    import torch
    ode = _ode(gpu, nx, norm)
    s = gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=7, F=tab, G='RK1', step_mode=mode)
    U0 = _states(nx, 5, 100 + nx)
    T0, T1 = _spans(5)
    got = s.run_F_batch(_t(torch, T0), _t(torch, T1), _t(torch, U0)).cpu().numpy()
    f = DiffReactNP(nx, normalized=norm)
    ref = np.array([rk_np(f, int(tab[2:]), T0[i], T1[i], 7, U0[i], mode) for i in range(5)])
    assert np.all(np.isfinite(got)) and np.array_equal(got, ref)


@pytest.mark.parametrize('nx', [16, 17, 32])
@pytest.mark.parametrize('n', [1, 5, 300])
@pytest.mark.parametrize('tab', ['RK1', 'RK2', 'RK4', 'RK8'])
def test_pair_kernel_is_bitwise_the_element_kernel(gpu, nx, n, tab, monkeypatch):
    """The default from 16x16 points (one thread per point) against the element-per-thread kernel
    that NNGP_RK_THREADS forces, both step modes, '-11' on the odd grid."""
    import torch
    ode = _ode(gpu, nx, nx == 17)
    U0 = _t(torch, _states(nx, n, 7 * nx + n))
    T0, T1 = _spans(n)
    T0, T1 = _t(torch, T0), _t(torch, T1)
    for mode in ('fixed', 'linspace'):
        s = gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=7, F=tab, G='RK1', step_mode=mode)
        monkeypatch.delenv('NNGP_RK_THREADS', raising=False)
        pair = s.run_F_batch(T0, T1, U0).cpu().numpy()
        monkeypatch.setenv('NNGP_RK_THREADS', FORCED_THREADS)
        elem = s.run_F_batch(T0, T1, U0).cpu().numpy()
        assert np.all(np.isfinite(pair)) and np.array_equal(pair, elem), mode


@pytest.mark.parametrize('key,nx,norm', [('4', 4, False), ('10_n', 10, True), ('17', 17, False)])
@pytest.mark.parametrize('tab', ['RK1', 'RK2', 'RK4', 'RK8'])
@pytest.mark.parametrize('mode', ['fixed', 'linspace'])
def test_rk_within_tolerance_of_reference(gpu, key, nx, norm, tab, mode):
    import torch
    R = golden('diffreact.npz')
    k = f'rk__{key}__{tab}'
    t0, t1, steps = R[k + '__span']
    s = gpu.SolverRK(_ode(gpu, nx, norm).get_vector_field(), Ng=int(steps), Nf=int(steps), F=tab, G=tab,
                     step_mode=mode)
    got = s.run_F_batch(_t(torch, [t0]), _t(torch, [t1]), _t(torch, R[k + '__u0'][None, :])).cpu().numpy()[0]
    ref = R[k + '__' + mode]
    assert np.max(np.abs(got - ref)) <= 1e-13 * max(1.0, np.max(np.abs(ref)))


@pytest.mark.parametrize('nx', [10, 17])
def test_rk_batch_grid_from_j0_zero_equals_linspace(gpu, nx):
    import torch
    from nngp_amd import _lib
    ode = _ode(gpu, nx, True)
    U0 = _t(torch, _states(nx, 5, nx))
    T0, T1 = _spans(5)
    T0, T1 = _t(torch, T0), _t(torch, T1)
    s = gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=7, F='RK4', G='RK1', step_mode='linspace')
    lin = s.run_F_batch(T0, T1, U0)
    out = torch.empty_like(U0)
    j0 = torch.zeros(5, dtype=torch.int64, device='cuda')
    cs = ode.get_vector_field().csystem(U0.device)
    _lib.check(_lib.lib().nngp_rk_batch_grid(ctypes.byref(cs), 4, 5, T0.data_ptr(), T1.data_ptr(), 7, j0.data_ptr(),
                                             7, U0.data_ptr(), out.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream))
    assert torch.equal(out, lin)


@pytest.mark.parametrize('nx', [10, 17])
@pytest.mark.parametrize('tab', ['RK1', 'RK2', 'RK4', 'RK8'])
def test_contracted_build_within_1e12_of_exact(gpu, nx, tab):
    import torch
    ode = _ode(gpu, nx, nx == 10)
    U0 = _t(torch, _states(nx, 5, nx))
    T0, T1 = _spans(5)
    T0, T1 = _t(torch, T0), _t(torch, T1)
    run = lambda fma: gpu.SolverRK(ode.get_vector_field(), Ng=1, Nf=40, F=tab, G='RK1',
                                   fma=fma).run_F_batch(T0, T1, U0).cpu().numpy()
    ex, fm = run(False), run(True)
    assert np.all(np.isfinite(fm))
    assert np.max(np.abs(fm - ex)) / max(1.0, np.max(np.abs(ex))) <= 1e-12


# ------------------------------------------------------------------------------------------------
# the layers above the propagator
# ------------------------------------------------------------------------------------------------
def _parareal(gpu, d_x, N, T, **kw):
    ode = gpu.DiffReact(d_x=d_x, normalization='-11')
    s = gpu.SolverRK(ode.get_vector_field(), Ng=2, Nf=40, F='RK4', G='RK1')
    return gpu.Parareal(ode, s, [0, T], N, epsilon=5e-7, verbose=None, **kw)


def _final(u):
    """the last computed iterate of a reference `u` [N+1][d][iterations] (NaN where not computed)"""
    cols = [c for c in range(u.shape[2]) if not np.any(np.isnan(u[:, :, c]))]
    return u[:, :, cols[-1]]


def _bound(R, d_x):
    """max(10 eps, 10 x the classic run's own distance from the serial fine solution): both models
    stop on the same eps = 5e-7 but along different iterates"""
    return max(5e-6, 10 * np.max(np.abs(_final(R[f'para__{d_x}__u']) - R[f'para__{d_x}__fine'])))


@pytest.mark.parametrize('d_x,N,T', [(4, 8, 4), (8, 16, 8)])
def test_classic_parareal_matches_reference(gpu, d_x, N, T):
    R = golden('diffreact.npz')
    r = _parareal(gpu, d_x, N, T).run(model='parareal')
    assert r['converged']
    assert r['k'] == int(R[f'para__{d_x}__k'])
    assert r['conv_int'] == list(R[f'para__{d_x}__conv_int'])
    assert np.nanmax(np.abs(r['u'] - R[f'para__{d_x}__u'])) < 1e-9


@pytest.fixture(scope='module')
def nngp_run(gpu):
    """nnGParareal on d_x = 4, N = 8, nn = 10, seed 45, speculation off: shared, left unchanged"""
    r = _parareal(gpu, 4, 8, 4, speculate=0).run(model='nngp', nn=10, seed=45)
    r['u'].setflags(write=False)
    return r


def _same(a, b):
    return np.array_equal(np.nan_to_num(a, nan=7.0), np.nan_to_num(b, nan=7.0))


def test_nngp_converges_to_the_fine_solution(gpu, nngp_run):
    R = golden('diffreact.npz')
    assert nngp_run['converged'] and nngp_run['k'] <= 8
    assert np.max(np.abs(nngp_run['u'][:, :, -1] - R['para__4__fine'])) <= _bound(R, 4)


def test_nngp_speculation_is_bitwise(gpu, nngp_run):
    r = _parareal(gpu, 4, 8, 4, speculate=1).run(model='nngp', nn=10, seed=45)
    assert r['k'] == nngp_run['k'] and r['conv_int'] == nngp_run['conv_int'] and _same(r['u'], nngp_run['u'])


def test_nngp_chain_knob_is_bitwise(gpu, nngp_run, monkeypatch):
    """no in-kernel G for DiffReact: NNGP_CHAIN=1 falls back to the launch chain"""
    monkeypatch.setenv('NNGP_CHAIN', '1')
    r = _parareal(gpu, 4, 8, 4, speculate=1).run(model='nngp', nn=10, seed=45)
    assert r['k'] == nngp_run['k'] and r['conv_int'] == nngp_run['conv_int'] and _same(r['u'], nngp_run['u'])


@pytest.mark.timeout(200)
def test_nngp_sharded_sweep_emulating_three_ranks_is_bitwise(gpu, nngp_run, tmp_path):
    """The coordinate-sharded sweep (nngp_correction_sweep_sharded_emulated: one process plays the
    3 ranks of the split of d = 32 into 11 + 11 + 10 coordinates), set up as
    tests/test_gpu_distributed.py does: a one-rank RCCL group in a child process."""
    out = str(tmp_path / 'shard.npz')
    code = r'''
import os, sys, socket
import numpy as np
import torch
sys.path.insert(0, os.environ["NNGP_ROOT"])
torch.cuda.set_device(0)
with socket.socket() as s:
    s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
torch.distributed.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                                     device_id=torch.device("cuda", 0))
import nngp_amd as g
from nngp_amd import _lib
assert _lib.comm_for(None)
os.environ["NNGP_SHARD_EMULATE_RANKS"] = "3"
ode = g.DiffReact(d_x=4, normalization="-11")
s = g.SolverRK(ode.get_vector_field(), Ng=2, Nf=40, F="RK4", G="RK1")
p = g.Parareal(ode, s, [0, 4], 8, epsilon=5e-7, verbose=None)
r = p.run(model="nngp", nn=10, seed=45, shard_corrections=True, native_comm=True)
np.savez(sys.argv[1], k=r["k"], conv=np.array(r["conv_int"]), u=r["u"])
torch.distributed.destroy_process_group()
print("shard ok")
'''
    p = subprocess.run([sys.executable, '-c', code, out], env=dict(os.environ, NNGP_ROOT=os.path.dirname(HERE)),
                       capture_output=True, text=True, timeout=180)
    assert p.returncode == 0 and 'shard ok' in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
    S = np.load(out)
    assert int(S['k']) == nngp_run['k'] and list(S['conv']) == list(nngp_run['conv_int'])
    assert _same(S['u'], nngp_run['u'])


def test_gparareal_converges_to_the_fine_solution(gpu):
    R = golden('diffreact.npz')
    r = _parareal(gpu, 4, 8, 4).run(model='gpjax')
    assert r['converged'] and r['k'] <= 8
    assert np.max(np.abs(r['u'][:, :, -1] - R['para__4__fine'])) <= _bound(R, 4)
