"""The measurement of DESIGN.md 3.3b (recorded, not gated; profiles/r18/predict_batch.txt): 511
independent nnGP predictions through one nngp_predict_batch call against the same 511 through the
per-query loop of predict_device (what Parareal._compare_models did).  Device events, warmed,
repeated, the sides alternated in one process; the outputs are compared bitwise.

    python tools/predict_batch_probe.py [output file]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nngp_amd as g                      # noqa: E402
from nngp_amd import _lib                 # noqa: E402

g.lib()
_lib.require_gpu()
dev = torch.device('cuda', 0)
out_lines = []
NQ = 511
# (d, m, rows, rounds); the single-correction fits per second of profiles/r06/bench.json
# (nngp_correction_roofline, rows = 3000) beside them where that file has the shape
SHAPES = [(3, 15, 2000, 7, None), (128, 15, 1000, 5, 2.16e6), (800, 20, 1000, 3, 3.78e6)]


def say(s):
    print(s, flush=True)
    out_lines.append(s)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)   # ms


def ab(fns, rounds):
    """median ms of each side, the sides alternated round by round after one warm-up each"""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            res[k].append(timed(f))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in res.items()}


def main():
    say('device: ' + torch.cuda.get_device_name(0))
    say(f'# one nngp_predict_batch call (n_q = {NQ}) against {NQ} x nngp_predict (NNGP_p.predict_device per query)')
    say('# ms per pass over the queries: median (min .. max) of alternated rounds x 1 pass, device events')
    for d, m, rows, rounds, r06 in SHAPES:
        rng = np.random.default_rng(rows + d)
        Xh = np.cumsum(0.05 * rng.standard_normal((rows, d)), axis=0)
        X = torch.tensor(Xh, device=dev)
        Y = torch.tensor(0.01 * np.sin(3 * Xh) + 1e-5 * rng.standard_normal(Xh.shape), device=dev)
        Q = (X[torch.tensor(rng.integers(0, rows, NQ), device=dev)] + 1e-2).contiguous()
        mdl = g.NNGP_p(n=d, N=4, nn=m, seed=45)
        mdl.fit(X, Y, 0)
        nf = mdl.n_fits
        th0 = torch.tensor(mdl.draw_thetas(NQ), dtype=torch.float64, device=dev)
        P1 = torch.empty((NQ, d), dtype=torch.float64, device=dev)
        P2 = torch.empty((NQ, d), dtype=torch.float64, device=dev)

        def batched():
            mdl.predict_batch_device(Q, theta0=th0, preds=P1)

        def loop():
            for j in range(NQ):
                mdl.predict_device(X, Y, rows, Q[j], th0[j * nf:(j + 1) * nf], preds=P2[j])

        r = ab({'batched': batched, 'loop': loop}, rounds)
        same = bool(torch.equal(P1.view(torch.int64), P2.view(torch.int64)))
        fps = lambda ms: NQ * nf / (ms * 1e-3)
        say(f'd={d:4d} m={m} rows={rows}  fits/query {nf:5d}  rounds {rounds}'
            f'  batched {r["batched"][0]:9.3f} ({r["batched"][1]:.3f} .. {r["batched"][2]:.3f})'
            f'   loop {r["loop"][0]:9.3f} ({r["loop"][1]:.3f} .. {r["loop"][2]:.3f})'
            f'   ratio {r["loop"][0] / r["batched"][0]:6.2f}x   bitwise equal {same}')
        say(f'       fits/s: batched {fps(r["batched"][0]):.3e}   loop {fps(r["loop"][0]):.3e}'
            + (f'   single correction, profiles/r06 {r06:.2e}' if r06 else ''))
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            f.write('\n'.join(out_lines) + '\n')


if __name__ == '__main__':
    main()
