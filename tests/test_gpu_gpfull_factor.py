"""GPU: the full-GP Cholesky factor itself (csrc/nngp_gpfull.hip through nngp_gpfull_factor), the
solves and the posterior mean against the backward-error bounds of tests/gpf_cases.py -- bounds
that depend on neither cond(K) nor the summation order and hold no measured number -- at every
panel, tile and launch edge, in every factor order, at d = 1, 3 and 200 and every jitter of
arange(-20, -11).  tests/test_gpf_cases_host.py shows on the CPU that LAPACK's factor is inside
every bound at every case here and that subtly wrong factors are far outside.

Every test prints its figures (the largest ratio to each bound) before it asserts."""
import ctypes

import numpy as np
import pytest

import gpf_cases as C

pytestmark = pytest.mark.gpu

_ip = ctypes.POINTER(ctypes.c_int32)
_dp = ctypes.POINTER(ctypes.c_double)


def _dev(torch, a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


def _args(pts):
    co = np.ascontiguousarray([p[3] for p in pts], dtype=np.int32)
    jx = np.ascontiguousarray([p[2] for p in pts], dtype=float)
    th = np.ascontiguousarray([p[:2] for p in pts], dtype=float).reshape(len(pts), 2)
    return co, jx, th


def _lml(gpu, torch, X, Y, pts):
    """nngp_gpfull_lml with the weights: (fval [nb], alpha [nb][n])."""
    n, d = X.shape
    co, jx, th = _args(pts)
    fv = np.empty(len(pts))
    al = torch.full((len(pts), n), float('nan'), dtype=torch.float64, device='cuda')
    gpu._lib.check(gpu.lib().nngp_gpfull_lml(X.data_ptr(), n, d, Y.data_ptr(), len(pts), co.ctypes.data_as(_ip),
                                             jx.ctypes.data_as(_dp), th.ctypes.data_as(_dp), fv.ctypes.data_as(_dp),
                                             al.data_ptr(), None))
    torch.cuda.synchronize()
    return fv, al.cpu().numpy()


def _factor(gpu, torch, X, Y, pts):
    """nngp_gpfull_factor: (fval, alpha, F [nb] of (n+1) x n trapezoids, fail [nb], D2 [n][n])."""
    n, d = X.shape
    nb = len(pts)
    co, jx, th = _args(pts)
    fv = np.empty(nb)
    al = torch.full((nb, n), float('nan'), dtype=torch.float64, device='cuda')
    A = torch.full((nb, n + 1, n + 1), float('nan'), dtype=torch.float64, device='cuda')
    fail = torch.full((nb,), -1, dtype=torch.int32, device='cuda')
    D2 = torch.full((n, n), float('nan'), dtype=torch.float64, device='cuda')
    gpu._lib.check(gpu.lib().nngp_gpfull_factor(X.data_ptr(), n, d, Y.data_ptr(), nb, co.ctypes.data_as(_ip),
                                                jx.ctypes.data_as(_dp), th.ctypes.data_as(_dp),
                                                fv.ctypes.data_as(_dp), al.data_ptr(), A.data_ptr(), fail.data_ptr(),
                                                D2.data_ptr(), None))
    torch.cuda.synchronize()
    A = A.cpu().numpy()
    return fv, al.cpu().numpy(), [C.trapezoid(A[b], n) for b in range(nb)], fail.cpu().numpy(), D2.cpu().numpy()


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_results(r, s, fail):
    """fval, and alpha and F of every point that did not fail, bit for bit."""
    ok = _same(r[0], s[0]) and np.array_equal(r[3], s[3])
    for b in np.flatnonzero(fail == 0):
        ok = ok and _same(r[1][b], s[1][b]) and _same(r[2][b], s[2][b])
    return ok


def _check_point(tag, F, fval, alpha, D2, pt, yv):
    """fail = 0: finite positive pivots and every bound; returns the factor's ratio to 2 gamma."""
    dg = np.diagonal(F[:F.shape[1]])
    assert np.all(np.isfinite(F)) and np.all(dg > 0), tag
    r = C.factor_check(F, D2, pt, yv)
    rl, ra = C.lml_check(F, fval), C.alpha_check(F, alpha)
    print(f'{tag}: factor {r["ratio"]:.3f} of its bound ({r["ratio_g"]:.3f} of 2 gamma_(n+1)), '
          f'-LML {rl:.3f}, alpha {ra:.3f}')
    assert r['ratio'] <= 1.0, (tag, r)
    assert rl <= 1.0, (tag, 'lml', rl)
    assert ra <= 1.0, (tag, 'alpha', ra)
    return r['ratio_g']


def _d2_checked(D2, x):
    assert _same(D2, C.d2_ref(x)), ('D2 is not bitwise scipy', C.d2_fallback_ratio(D2, x))
    return D2


def _run_case(gpu, torch, monkeypatch, order, x, y, pts, n_bad=0):
    """One batch through nngp_gpfull_lml / nngp_gpfull_factor / nngp_gpfull_lml again (bitwise
    each other), under NNGP_GPF_FUSE=0 and one matrix per slab chunk (bitwise on F); then every
    bound on every point that is expected to factor.  The last n_bad points are NaN points."""
    for k, v in C.ORDERS[order].items():
        monkeypatch.setenv(k, v)
    n, d = x.shape
    X, Y = _dev(torch, x), _dev(torch, y)
    before = _lml(gpu, torch, X, Y, pts)
    r = _factor(gpu, torch, X, Y, pts)
    after = _lml(gpu, torch, X, Y, pts)
    fv, al, Fs, fail, D2 = r
    good = len(pts) - n_bad
    assert list(fail) == [0] * good + [1] * n_bad, fail
    assert np.all(np.isposinf(fv[good:]))
    for o in (before, after):   # the diagnostic entry changes nothing nngp_gpfull_lml returns
        assert _same(o[0], fv) and _same(o[1][:good], al[:good])
    _d2_checked(D2, x)
    if order != 'rl32':
        monkeypatch.setenv('NNGP_GPF_FUSE', '0')
        assert _same_results(_factor(gpu, torch, X, Y, pts), r, fail), 'NNGP_GPF_FUSE=0 differs'
        monkeypatch.delenv('NNGP_GPF_FUSE')
    per = 8 * (n + 1) ** 2
    mb = max(1, per >> 20)
    if max(1, (mb << 20) // per) < len(pts):   # the smallest slab (1 MB) holds every matrix below n ~ 210
        monkeypatch.setenv('NNGP_GPF_SLAB_MB', str(mb))
        assert _same_results(_factor(gpu, torch, X, Y, pts), r, fail), 'slab chunks differ'
        monkeypatch.delenv('NNGP_GPF_SLAB_MB')
    else:
        assert n < 257
    worst = 0.0
    for b in range(good):
        sx, sy, jit, co = pts[b]
        worst = max(worst, _check_point(f'{order} n={n} d={d} sx={sx} jit={jit}', Fs[b], fv[b], al[b], D2,
                                        C.gp_point(sx, sy, jit), np.ascontiguousarray(y[:, co])))
    return worst


@pytest.mark.parametrize('order', sorted(C.ORDERS))
@pytest.mark.parametrize('n', C.SIZES)
def test_factor_is_backward_stable_at_every_edge(gpu, n, order, monkeypatch):
    """Panel edges of both widths (31/32/33, 63/64/65, 127/128/129, 191/192/193), the row-solve
    block edge (319/320/321) and 1, 2, 257: the cond >= 1e10 point, the cond <= 1e4 point and a
    NaN point (sigma_x = 0, which must fail) in one batch."""
    import torch
    x, y = C.data(n, 3)
    w = _run_case(gpu, torch, monkeypatch, order, x, y, C.size_points(n) + [C.NAN_POINT], n_bad=1)
    print(f'{order} n={n}: largest |R| / (2 gamma_(n+1) |L||L^T|) = {w:.3f}')


@pytest.mark.parametrize('order', sorted(C.ORDERS))
def test_factor_at_600_rows(gpu, order, monkeypatch):
    """The size GParareal reaches (cond(K) = 2.7e14), one point per order."""
    import torch
    x, y = C.data(C.BIG, 3)
    w = _run_case(gpu, torch, monkeypatch, order, x, y, C.size_points(C.BIG)[:1] + [C.NAN_POINT], n_bad=1)
    print(f'{order} n={C.BIG}: largest |R| / (2 gamma_(n+1) |L||L^T|) = {w:.3f}')


@pytest.mark.parametrize('order', sorted(C.ORDERS))
@pytest.mark.parametrize('d', C.DIM_DS)
@pytest.mark.parametrize('n', C.DIM_NS)
def test_factor_at_every_dimension_and_jitter(gpu, n, d, order, monkeypatch):
    """d = 1, 3 and 200 (the stalled FHN-PDE d_x = 10 row has d = 200), cond(K) >= 1e10, every
    jitter of arange(-20, -11), coordinates 0 and d - 1 among them."""
    import torch
    x, y = C.data(n, d)
    w = _run_case(gpu, torch, monkeypatch, order, x, y, C.dim_points(n, d))
    print(f'{order} n={n} d={d}: largest |R| / (2 gamma_(n+1) |L||L^T|) = {w:.3f}')


@pytest.mark.parametrize('order', sorted(C.ORDERS))
def test_batch_shapes_do_not_change_a_point(gpu, order, monkeypatch):
    """nb = 1, 2, 3, 7, 8, 9 (two matrices per wave in the right-looking diagonal kernel, grids
    padded to 8): every point's F, fval and alpha are bitwise what the point gives alone, also
    with a NaN point in each position in turn (both halves of a wave)."""
    import torch
    for k, v in C.ORDERS[order].items():
        monkeypatch.setenv(k, v)
    x, y = C.data(C.BATCH_N, 3)
    X, Y = _dev(torch, x), _dev(torch, y)
    pool = C.batch_points(max(C.BATCH_NBS))
    alone = [_factor(gpu, torch, X, Y, [p]) for p in pool]
    assert all(a[3][0] == 0 for a in alone)

    def same_as_alone(r, b, p):
        a = alone[pool.index(p)]
        return r[3][b] == 0 and r[0][b].tobytes() == a[0][0].tobytes() and _same(r[1][b], a[1][0]) and \
            _same(r[2][b], a[2][0])

    for nb in C.BATCH_NBS:
        pts = C.batch_points(nb)
        r = _factor(gpu, torch, X, Y, pts)
        assert all(same_as_alone(r, b, p) for b, p in enumerate(pts)), nb
        for pos in range(nb):
            q = list(pts)
            q[pos] = C.NAN_POINT
            r = _factor(gpu, torch, X, Y, q)
            assert r[3][pos] == 1 and np.isposinf(r[0][pos]), (nb, pos)
            assert all(same_as_alone(r, b, p) for b, p in enumerate(q) if b != pos), (nb, pos)


@pytest.mark.parametrize('order', sorted(C.ORDERS))
def test_failure_is_self_consistent(gpu, order, monkeypatch):
    """A duplicated row at jitter -20: the second pivot is rounding noise, so which way it goes is
    not asserted -- fail = 0 means finite positive pivots and every bound, fail = 1 means +inf."""
    import torch
    for k, v in C.ORDERS[order].items():
        monkeypatch.setenv(k, v)
    x, y, pts = C.duplicate_case()
    fv, al, Fs, fail, D2 = _factor(gpu, torch, _dev(torch, x), _dev(torch, y), pts)
    print(f'{order}: duplicated row, fail = {fail[0]}, fval = {fv[0]}')
    assert fail[0] in (0, 1)
    if fail[0]:
        assert np.isposinf(fv[0])
    else:
        sx, sy, jit, co = pts[0]
        _check_point(f'{order} duplicated row', Fs[0], fv[0], al[0], _d2_checked(D2, x), C.gp_point(sx, sy, jit),
                     np.ascontiguousarray(y[:, co]))


@pytest.mark.parametrize('d', C.MEAN_DS)
@pytest.mark.parametrize('n', C.MEAN_NS)
def test_posterior_mean_is_inside_its_bound(gpu, n, d):
    """gpf_mean_kernel at the 256-thread stride's edges and 1 / 600 rows, d = 1, 3, 200, weights of
    magnitude 1e-3..1e10 with mixed signs, with and without the bias."""
    import torch
    x, q, coef, alpha, bias = C.mean_case(n, d)
    X, Q, Cf, Al, Bi = (_dev(torch, a) for a in (x, q, coef, alpha, bias))
    for b, B in ((None, None), (bias, Bi)):
        out = torch.full((d,), float('nan'), dtype=torch.float64, device='cuda')
        gpu._lib.check(gpu.lib().nngp_gpfull_mean(X.data_ptr(), n, d, Q.data_ptr(), Cf.data_ptr(), Al.data_ptr(),
                                                  B.data_ptr() if B is not None else None, out.data_ptr(), None))
        torch.cuda.synchronize()
        ref, bnd = C.mean_reference(x, q, coef, alpha, b)
        ratio = np.abs(out.cpu().numpy().astype(C.LD) - ref) / bnd
        print(f'mean n={n} d={d} bias={b is not None}: {float(ratio.max()):.3f} of its bound')
        assert np.all(ratio <= 1.0), (n, d, float(ratio.max()))
