"""Cost of an adaptive step (nngp_rk_adaptive) per right-hand-side evaluation,
beside the same systems' fixed-step RK4 kernels (nngp_rk_batch) measured in the same run.

    python tools/adaptive_probe.py [--reps R] [--evals E]

  lane:  Lorenz, '-11', 128 slices
  field: FHN-PDE d = 800 (d_x = 20), '-11', 64 and 512 slices
For each, RK45 in two regimes -- 'capped': rtol 1e-3 with nf so large that every step is max_step
(all slices take the same steps); 'controlled': rtol 1e-8, nf = 1, the controller sizes every step
and the slices differ -- and RK4 with the same number of evaluations (E, default 24000 per slice).
A launch ends with its slowest slice, so the adaptive figure is device time over the LARGEST nfev of
the launch; the per-slice spread of nfev is printed beside it.  Each launch is timed with events
after two warm-up launches; every time is printed, then the median.
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), ms


def report(label, med, ms, evals, extra=''):
    print(f'{label}: median {med:.3f} ms / {evals} evaluations = {med * 1e3 / evals:.5f} us/evaluation  '
          f'min {min(ms):.3f} max {max(ms):.3f}  all [{", ".join(f"{x:.3f}" for x in ms)}]{extra}', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--evals', type=int, default=24000)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import nngp_amd as g
    from nngp_amd import _lib
    torch.cuda.set_device(0)
    L = _lib.lib()
    rng = np.random.default_rng(0)
    stream = torch.cuda.current_stream().cuda_stream

    def adaptive(ode, n, length, rtol, atol, nf, label):
        d = ode.get_dim()
        U0 = dev(ode.get_init_cond()[None, :] + 0.01 * rng.standard_normal((n, d)))
        T0 = dev(np.linspace(0, 1, n))
        T1 = T0 + length
        out = torch.empty_like(U0)
        stats = torch.zeros((n, 4), dtype=torch.int64, device='cuda')
        cs = ode.get_vector_field().csystem(U0.device)

        def fn():
            _lib.check(L.nngp_rk_adaptive(ctypes.byref(cs), 45, n, T0.data_ptr(), T1.data_ptr(), nf, rtol, atol, 0.0,
                                          100 * nf + 10 ** 7, U0.data_ptr(), out.data_ptr(), stats.data_ptr(), stream))
        med, ms = timed(fn, a.reps)
        st = stats.cpu().numpy()
        assert np.all(st[:, 0] == 0), st[:, 0]
        report(label, med, ms, int(st[:, 1].max()),
               f'  nfev {st[:, 1].min()}..{st[:, 1].max()} mean {st[:, 1].mean():.0f}, rejected {st[:, 3].sum()}')

    def fixed(ode, n, length, steps, label):
        d = ode.get_dim()
        U0 = dev(ode.get_init_cond()[None, :] + 0.01 * rng.standard_normal((n, d)))
        T0 = dev(np.linspace(0, 1, n))
        T1 = T0 + length
        s = g.SolverRK(ode.get_vector_field(), Ng=4, Nf=steps, F='RK4', G='RK1')
        out = torch.empty_like(U0)
        med, ms = timed(lambda: s.run_F_batch(T0, T1, U0, out=out), a.reps)
        report(label, med, ms, 4 * steps)

    E = a.evals
    lorenz = g.Lorenz(normalization='-11')
    fixed(lorenz, 128, 1.0, E // 4, 'Lorenz n=128 fixed RK4 (default kernel)')
    os.environ['NNGP_RK_GROUP'] = '0'
    fixed(lorenz, 128, 1.0, E // 4, 'Lorenz n=128 fixed RK4 (lane kernel)   ')
    del os.environ['NNGP_RK_GROUP']
    adaptive(lorenz, 128, 1.0, 1e-3, 1e-6, E // 6, 'Lorenz n=128 RK45 capped              ')
    adaptive(lorenz, 128, 40.0, 1e-8, 1e-11, 1, 'Lorenz n=128 RK45 controlled          ')
    fhn = g.FHN_PDE(d_x=20, normalization='-11')
    for n in (64, 512):
        fixed(fhn, n, 1.0, E // 4, f'FHN-PDE d=800 n={n} fixed RK4 (default kernel)')
        os.environ['NNGP_FHN_PAIR'] = '0'
        fixed(fhn, n, 1.0, E // 4, f'FHN-PDE d=800 n={n} fixed RK4 (element kernel)')
        del os.environ['NNGP_FHN_PAIR']
        adaptive(fhn, n, 1.0, 1e-3, 1e-6, E // 6, f'FHN-PDE d=800 n={n} RK45 capped              ')
        adaptive(fhn, n, 400.0, 1e-8, 1e-11, 1, f'FHN-PDE d=800 n={n} RK45 controlled          ')


if __name__ == '__main__':
    main()
