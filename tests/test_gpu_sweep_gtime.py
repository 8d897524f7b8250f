"""The G-time measurement of the four local correction sweeps (GTimer, csrc/common.h) at its edges.

nngp_correction_sweep (Parareal; nnGParareal without speculation), nngp_elm_sweep and
nngp_knn_mean_sweep over N - I = 0, 1, 8, 9 and 17 slices -- the empty sweep, one timed slice, and
exactly, one over and two over the default stride of 8 -- with NNGP_G_TIME_EVERY unset, 1 and 3, with
and without g_ms_out: the timing never changes what the sweep computes or where it writes, and the
time is 0 for an empty sweep and positive otherwise.  Lorenz (d = 3), RK1 G of 5 steps, 40 training
rows; what the sweeps compute is pinned to the oracle by the per-model test files."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, I, NG, ROWS, M, RES = 3, 3, 5, 40, 5, 8
N_MAX = I + 17
SENTINEL = -7.0
SLICES = [0, 1, 8, 9, 17]
STRIDES = [None, '1', '3']

_DATA = {}


def _data(gpu):
    """The shared inputs, on the device, built once and never written."""
    if _DATA:
        return _DATA
    import torch
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')
    ode = gpu.Lorenz(normalization='-11')
    solver = gpu.SolverRK(ode.get_vector_field(), Ng=NG, Nf=50, F='RK4', G='RK1')
    rng = np.random.default_rng(17)
    u0 = np.asarray(ode.get_init_cond(), dtype=np.float64)
    X = u0 + 0.05 * rng.standard_normal((ROWS, D))
    Y = 1e-3 * rng.standard_normal((ROWS, D))
    U = u0 + 0.01 * rng.standard_normal((N_MAX + 1, D))
    bias_h, C = rng.standard_normal(RES), rng.standard_normal((RES, 1 + D))
    _DATA.update(solver=solver, cs=solver.f.csystem(torch.device('cuda', torch.cuda.current_device())),
                 t=dev(np.linspace(0.0, 0.02 * N_MAX, N_MAX + 1)), U=U, X=dev(X), Y=dev(Y),
                 UF=dev(U + 1e-3 * rng.standard_normal(U.shape)), UG=dev(U + 1e-3 * rng.standard_normal(U.shape)),
                 th0=dev(gpu.NNGP_p(n=D, N=4, nn=M, seed=3).draw_thetas(17)), bias_h=dev(bias_h), C=dev(C),
                 H=torch.zeros((ROWS, RES), dtype=torch.float64, device='cuda'),
                 scratch=torch.empty(D, dtype=torch.float64, device='cuda'))
    st = torch.cuda.current_stream().cuda_stream
    gpu._lib.check(gpu.lib().nngp_elm_hidden(_DATA['X'].data_ptr(), ROWS, D, 1, RES, _DATA['bias_h'].data_ptr(),
                                             _DATA['C'].data_ptr(), _DATA['H'].data_ptr(), st))
    torch.cuda.synchronize()
    return _DATA


def _run(gpu, entry, N, with_g_ms):
    """One sweep I .. N-1 from fresh buffers: (rc, U1, UG1, g_ms or None, U1 as it was)."""
    import torch
    S, L = _data(gpu), gpu.lib()
    U0 = np.where(np.arange(N_MAX + 1)[:, None] <= I, S['U'], SENTINEL)
    U1 = torch.tensor(U0, dtype=torch.float64, device='cuda')
    UG1 = torch.full((N_MAX + 1, D), SENTINEL, dtype=torch.float64, device='cuda')
    g_ms = ctypes.c_float(-1.0)
    g_ref = ctypes.byref(g_ms) if with_g_ms else None
    st = torch.cuda.current_stream().cuda_stream
    head = (ctypes.byref(S['cs']), gpu._lib.TABLEAU['RK1'], S['solver'].step_mode, NG, S['t'].data_ptr(), I, N,
            U1.data_ptr(), UG1.data_ptr())
    if entry == 'parareal':
        rc = L.nngp_correction_sweep(*head, S['UF'].data_ptr(), S['UG'].data_ptr(), gpu._lib.MODEL_PARAREAL, None, None,
                                     0, 0, 0, None, 0, None, 0.0, 0.0, 0, None, 0, None, g_ref, st)
    elif entry == 'nngp':
        jit, jp = gpu._lib.host_doubles(np.arange(-20, -11, dtype=float))
        rc = L.nngp_correction_sweep(*head, S['UF'].data_ptr(), S['UG'].data_ptr(), gpu._lib.MODEL_NNGP,
                                     S['X'].data_ptr(), S['Y'].data_ptr(), ROWS, M, len(jit), jp, 1, S['th0'].data_ptr(),
                                     0.1, 0.1, 400, S['scratch'].data_ptr(), 0, None, g_ref, st)
    elif entry == 'elm':
        rc = L.nngp_elm_sweep(*head, S['X'].data_ptr(), S['Y'].data_ptr(), S['H'].data_ptr(), ROWS, M, 1, RES,
                              S['bias_h'].data_ptr(), S['C'].data_ptr(), g_ref, st)
    else:
        rc = L.nngp_knn_mean_sweep(*head, S['X'].data_ptr(), S['Y'].data_ptr(), ROWS, M, None, g_ref, st)
    torch.cuda.synchronize()
    return rc, U1.cpu().numpy(), UG1.cpu().numpy(), (g_ms.value if with_g_ms else None), U0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# N = I - 1: an empty sweep for nngp_knn_mean_sweep only (the others refuse it)
CASES = [(e, n) for e in ('parareal', 'nngp', 'elm', 'knn') for n in SLICES] + [('knn', -1)]


@pytest.mark.parametrize('entry,n', CASES)
def test_g_time_leaves_the_sweep_alone(gpu, entry, n, monkeypatch):
    N = I + n
    first = None
    for stride in STRIDES:
        if stride is None:
            monkeypatch.delenv('NNGP_G_TIME_EVERY', raising=False)
        else:
            monkeypatch.setenv('NNGP_G_TIME_EVERY', stride)
        for with_g_ms in (True, False):
            rc, U1, UG1, g_ms, U0 = _run(gpu, entry, N, with_g_ms)
            print(f'{entry} slices={n} NNGP_G_TIME_EVERY={stride} g_ms={g_ms}')
            assert rc == 0, (rc, gpu.lib().nngp_last_error())
            # rows <= I (and past N) are untouched
            assert np.array_equal(_bits(U1[:I + 1]), _bits(U0[:I + 1])) and np.all(UG1[:I + 1] == SENTINEL)
            lo = max(N, I) + 1
            assert np.all(U1[lo:] == SENTINEL) and np.all(UG1[lo:] == SENTINEL)
            assert np.all(np.isfinite(U1[I + 1:lo])) and np.all(U1[I + 1:lo] != SENTINEL)
            assert np.all(np.isfinite(UG1[I + 1:lo])) and np.all(UG1[I + 1:lo] != SENTINEL)
            if first is None:
                first = (U1, UG1)
            assert np.array_equal(_bits(U1[I + 1:]), _bits(first[0][I + 1:]))
            assert np.array_equal(_bits(UG1[I + 1:]), _bits(first[1][I + 1:]))
            if with_g_ms:
                assert (g_ms == 0.0) if n <= 0 else (np.isfinite(g_ms) and g_ms > 0.0), g_ms
