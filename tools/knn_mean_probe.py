"""The measurements of DESIGN.md 3.7 (recorded, not gated; profiles/r12/knn_mean.txt): one nngp_knn_mean
call against the per-query loop, and the k-NN sweep per slice against the ELM and classic sweeps.
Device events, warmed, repeated, the sides alternated in one process.

    python tools/knn_mean_probe.py [output file]
"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nngp_amd as g                      # noqa: E402
from nngp_amd import _lib                 # noqa: E402

L = g.lib()
_lib.require_gpu()
dev = torch.device('cuda', 0)
out_lines = []


def say(s):
    print(s, flush=True)
    out_lines.append(s)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps   # ms


def ab(fns, rounds=7, reps=3):
    """median ms of each side, the sides alternated round by round after one warm-up each"""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            res[k].append(timed(f, reps))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in res.items()}


COUNTS = [1, 2, 3, 4, 5, 10, 15, 30]


def part_batched():
    say('# A. one nngp_knn_mean call (n_q = 511, counts %s) against 511 x (nngp_knn + torch gather-and-mean)' % COUNTS)
    rounds, reps = 5, 2
    say(f'# ms per call: median (min .. max) of {rounds} alternated rounds x {reps} calls, device events')
    st = torch.cuda.current_stream().cuda_stream
    cnt = torch.tensor(COUNTS, device=dev)
    for rows in (1500, 10000):
        for d in (3, 800):
            rng = np.random.default_rng(rows + d)
            X = torch.tensor(rng.standard_normal((rows, d)), device=dev)
            Y = torch.tensor(rng.standard_normal((rows, d)), device=dev)
            Q = X[torch.tensor(rng.integers(0, rows, 511), device=dev)] + 1e-2
            Q = Q.contiguous()
            mdl = g.NN(N=4, nn=30)
            mdl.fit(X, Y, 0)
            out = torch.empty((len(COUNTS), 511, d), dtype=torch.float64, device=dev)
            idx = torch.empty(30, dtype=torch.int32, device=dev)
            out2 = torch.empty((len(COUNTS), 511, d), dtype=torch.float64, device=dev)

            def batched():
                mdl.predict_batch_device(Q, counts=COUNTS, out=out)

            def loop():
                for j in range(511):
                    _lib.check(L.nngp_knn(X.data_ptr(), rows, d, Q[j].data_ptr(), 30, idx.data_ptr(), None, st))
                    cs = torch.cumsum(Y[idx.long()], dim=0)
                    out2[:, j] = cs[cnt - 1] / cnt[:, None]

            r = ab({'batched': batched, 'loop': loop}, rounds=rounds, reps=reps)
            close = float((out - out2).abs().max())
            say(f'rows={rows:6d} d={d:4d}  batched {r["batched"][0]:9.3f} ({r["batched"][1]:.3f} .. {r["batched"][2]:.3f})'
                f'   loop {r["loop"][0]:9.3f} ({r["loop"][1]:.3f} .. {r["loop"][2]:.3f})'
                f'   ratio {r["loop"][0] / r["batched"][0]:7.1f}x   max |diff| {close:.1e}')


def sweep_case(name, ode, solver, tspan, N):
    n = ode.get_dim()
    st = torch.cuda.current_stream().cuda_stream
    t_dev = torch.tensor(np.linspace(tspan[0], tspan[1], N + 1), dtype=torch.float64, device=dev)
    UG = torch.empty((N + 1, n), dtype=torch.float64, device=dev)
    UG[0] = torch.tensor(ode.get_init_cond(), dtype=torch.float64, device=dev)
    solver.initial_coarse(t_dev, UG, N)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(UG).all())
    rng = np.random.default_rng(1)
    # a training set like the second iteration's: two rows per slice around the coarse solution
    X = torch.cat([UG[:N], UG[:N] + 1e-3 * torch.tensor(rng.standard_normal((N, n)), device=dev)]).contiguous()
    Y = (1e-3 * torch.tensor(rng.standard_normal((2 * N, n)), device=dev)).contiguous()
    rows = 2 * N
    UF = UG + 1e-3
    U1, UG1 = UG.clone(), UG.clone()
    cs = solver.f.csystem(dev)
    tab, mode, Ng = _lib.TABLEAU[solver.G], solver.step_mode, solver.Ng
    I = 1
    elm = g.ELM(d=n, N=N)
    elm.ELM.weights_device(dev)
    elm.fit(X, Y, 0)
    Xe, Ye, He, rows_e = elm.ELM.device_state()
    be, Ce = elm.ELM.weights_device(dev)

    def knn():
        U1.copy_(UG)
        _lib.check(L.nngp_knn_mean_sweep(ctypes.byref(cs), tab, mode, Ng, t_dev.data_ptr(), I, N, U1.data_ptr(),
                                         UG1.data_ptr(), X.data_ptr(), Y.data_ptr(), rows, 3, None, None, st))

    def elm_sweep():
        U1.copy_(UG)
        e = elm.ELM
        _lib.check(L.nngp_elm_sweep(ctypes.byref(cs), tab, mode, Ng, t_dev.data_ptr(), I, N, U1.data_ptr(),
                                    UG1.data_ptr(), Xe.data_ptr(), Ye.data_ptr(), He.data_ptr(), rows_e,
                                    min(int(e.m), rows_e), e.poly_degree, e.N, be.data_ptr(), Ce.data_ptr(), None, st))

    def classic():
        U1.copy_(UG)
        _lib.check(L.nngp_correction_sweep(
            ctypes.byref(cs), tab, mode, Ng, t_dev.data_ptr(), I, N, U1.data_ptr(), UG1.data_ptr(), UF.data_ptr(),
            UG.data_ptr(), _lib.MODEL_PARAREAL, None, None, 0, 0, 0, None, 0, None, 0.0, 0.0, 0, None, 0, None, None, st))

    rounds, reps = 7, 3
    r = ab({'knn': knn, 'elm': elm_sweep, 'classic': classic}, rounds=rounds, reps=reps)
    per = lambda k: 1e3 * r[k][0] / (N - I)
    say(f'{name}: N={N} d={n} rows={rows}  us per slice (median of {rounds} alternated rounds x {reps} sweeps): '
        f'k-NN {per("knn"):8.1f}   ELM {per("elm"):8.1f}   classic {per("classic"):8.1f}')


def part_sweeps():
    say('# B. the sequential sweep per slice: nngp_knn_mean_sweep (m = 3) against nngp_elm_sweep and the classic sweep')
    ode = g.Lorenz(normalization='-11')
    s = g.SolverRK(ode.get_vector_field(), Ng=6, Nf=450, F='RK4', G='RK4')
    sweep_case('Lorenz', ode, s, [0, 18], 32)
    ode = g.FHN_PDE(d_x=20)
    # the benchmark's coarse solver (bench.py fhn_pde_converge): RK4 with 50 steps per slice
    s = g.SolverRK(ode.get_vector_field(), Ng=50, Nf=100, F='RK8', G='RK4', thresh=float('inf'))
    sweep_case('FHN-PDE', ode, s, [0, 1100], 512)


if __name__ == '__main__':
    say('device: ' + torch.cuda.get_device_name(0))
    part_batched()
    part_sweeps()
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            f.write('\n'.join(out_lines) + '\n')
