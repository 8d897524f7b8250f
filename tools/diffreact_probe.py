"""GPU probe: DiffReact d = 800 (d_x = 20) fine sweep, us per RK8 step at 512 and 64 slices, the
point-pair kernel (default) and the element kernel (NNGP_RK_THREADS), with FHN-PDE d_x = 20 timed
beside them in the same process on the same build (its point-pair kernel moves the same LDS
traffic per stage).  The variants alternate, `rounds` times, so that drift shows as spread.

    python tools/diffreact_probe.py [steps] [reps] [rounds] [out.txt]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nngp_amd as g  # noqa: E402


def make(system, n_sl, steps):
    if system == 'fhn':
        ode = g.FHN_PDE(d_x=20)
        span = 1100 / 512   # BASELINE configs[4]'s slice
    else:
        ode = g.DiffReact(d_x=20)
        span = 2e-3 * steps  # h = 2e-3: inside the explicit stability limit (Dv * 4/dx^2 = 2)
    s = g.SolverRK(ode.get_vector_field(), Ng=50, Nf=steps, F='RK8', G='RK4', thresh=float('inf'))
    rng = np.random.default_rng(0)
    U = np.clip(ode.get_init_cond()[None, :] + 0.01 * rng.standard_normal((n_sl, 800)), 0, 1)
    dev = lambda a: torch.tensor(a, dtype=torch.float64, device='cuda')
    t0 = span * np.arange(n_sl)
    return s, dev(t0), dev(t0 + span), dev(U)


def sweep_us(system, threads, n_sl, steps, reps):
    """best of `reps` timed sweeps after one warm-up sweep of the same shape"""
    if threads:
        os.environ['NNGP_RK_THREADS'] = threads
    else:
        os.environ.pop('NNGP_RK_THREADS', None)
    s, t0, t1, u0 = make(system, n_sl, steps)
    out = torch.empty_like(u0)
    s.run_F_batch(t0, t1, u0, out=out)
    torch.cuda.synchronize()
    best = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        s.run_F_batch(t0, t1, u0, out=out)
        b.record()
        b.synchronize()
        best.append(a.elapsed_time(b) * 1e3 / steps)
    os.environ.pop('NNGP_RK_THREADS', None)
    return min(best), float(out.sum().item())


if __name__ == '__main__':
    torch.cuda.set_device(0)
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    sink = open(sys.argv[4], 'w') if len(sys.argv) > 4 else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + '\n')
            sink.flush()

    say(f'# us per RK8 step, d = 800 (d_x = 20), {steps} steps per sweep, best of {reps}, {rounds} alternating rounds')
    # element kernel layouts: the default pick at d = 800 is 832 threads x 1 (few slices) or 512 x 2
    variants = [('fhn pair', 'fhn', ''), ('diffreact pair', 'dr', ''), ('diffreact element 832x1', 'dr', '832'),
                ('diffreact element 512x2', 'dr', '512'), ('diffreact element 256x4', 'dr', '256')]
    for n_sl in (512, 64):
        res = {v[0]: [] for v in variants}
        for _ in range(rounds):
            for name, system, thr in variants:
                us, ck = sweep_us(system, thr, n_sl, steps, reps)
                res[name].append(us)
                say(f'{n_sl} slices  {name:26s} {us:7.3f} us/step  checksum {ck:.17g}')
        for name, v in res.items():
            say(f'== {n_sl} slices  {name:26s} min {min(v):.3f}  max {max(v):.3f}')
        f, d = min(res['fhn pair']), min(res['diffreact pair'])
        say(f'== {n_sl} slices  diffreact pair / fhn pair = {d / f:.3f} (target <= 1.10)')
    if sink:
        sink.close()
