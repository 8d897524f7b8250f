"""CPU: the checker of tests/test_gpu_gpfull_factor.py has teeth, and the reference alone stays
inside its bounds (tests/gpf_cases.py).

- every case's LAPACK factor (np.linalg.cholesky / solve_triangular, as oracle/gpfull.py) passes
  every bound -- the condition that the inputs are fair: 100 % of the cases, none skipped for
  conditioning;
- a plain numpy restatement of the blocked left-looking order (64-column panels, k depth 4,
  reciprocal multiply, with and without FMA) passes too;
- mutants of that restatement (a k block dropped from one 16x16 sub-tile, the y row's update
  skipped for a panel, a short panel's last column unsolved, L_jj stored one update early) exceed
  the factor bound by >= 100x at the cond >= 1e10 point of n = 129 and n = 321, and a single entry
  moved by 64 gamma_{n+1} of its row's |L||L^T| scale fails."""
import numpy as np
import pytest

import gpf_cases as C


def _check_all(F, alpha, D2, pt, yv, tag):
    r = C.factor_check(F, D2, pt, yv)
    assert r['ratio'] <= 1.0, (tag, r)
    assert C.lml_check(F, C.lml_double(F)) <= 1.0, tag
    assert C.alpha_check(F, alpha) <= 1.0, tag
    return r


def _cases():
    for n in C.SIZES + (C.BIG,):
        yield pytest.param(n, 3, 'size', id=f'size-{n}')
    for n in C.DIM_NS:
        for d in C.DIM_DS:
            yield pytest.param(n, d, 'dim', id=f'dim-{n}-{d}')


@pytest.mark.parametrize('n,d,kind', _cases())
def test_lapack_and_restated_factors_are_inside_every_bound(n, d, kind):
    x, y, D2 = C.host_case(n, d)
    pts = C.size_points(n) if kind == 'size' else C.dim_points(n, d)
    conds = [C.cond_of(x, p[:2], p[2]) for p in pts]
    print(f'n={n} d={d} cond(K):', ' '.join(f'{c:.2e}' for c in conds))
    if kind == 'size' and n > 1:   # n = 1: cond(K) = 1 whatever theta is
        assert conds[0] >= 1e10 and conds[1] <= 1e4, conds
    if kind == 'dim':
        assert min(conds) >= 1e10, conds
        assert {p[3] for p in pts} >= {0, d - 1}
    worst = 0.0
    for (sx, sy, jit, co) in pts:
        pt, yv = C.gp_point(sx, sy, jit), np.ascontiguousarray(y[:, co])
        F, alpha = C.lapack_factor(D2, pt, yv)
        assert F is not None, ('LAPACK fails', n, d, sx, sy, jit)
        worst = max(worst, _check_all(F, alpha, D2, pt, yv, ('lapack', n, d, sx, jit))['ratio_g'])
        if kind == 'size' or jit in (-20.0, -12.0):   # the restated order: every size, the jitters' ends
            for fma in (False, True):
                G = C.restated_ll64(D2, pt, yv, fma=fma)
                assert G is not None
                _check_all(G, _alpha_of(G), D2, pt, yv, ('restated', fma, n, d, sx, jit))
    print(f'n={n} d={d} LAPACK max |R| / (2 gamma_(n+1) |L||L^T|) = {worst:.3f}')


def _alpha_of(F):
    import scipy.linalg
    n = F.shape[1]
    return scipy.linalg.solve_triangular(F[:n].T, F[n], lower=False)


@pytest.mark.parametrize('n', [129, 321])
def test_mutants_are_far_outside_the_factor_bound(n):
    x, y, D2 = C.host_case(n, 3)
    sx, sy, jit, co = C.size_points(n)[0]
    assert C.cond_of(x, (sx, sy), jit) >= 1e10
    pt, yv = C.gp_point(sx, sy, jit), np.ascontiguousarray(y[:, co])
    for fma in (False, True):
        good = C.restated_ll64(D2, pt, yv, fma=fma)
        assert C.factor_check(good, D2, pt, yv)['ratio'] <= 1.0
        for m in C.MUTANTS:
            G = C.restated_ll64(D2, pt, yv, fma=fma, mutant=m)
            assert G is not None and not np.array_equal(G, good), m
            r = C.factor_check(G, D2, pt, yv)
            print(f'n={n} fma={fma} {m}: {r["ratio"]:.3g} x the bound at {r["where"]}')
            assert r['ratio'] >= 100.0, (m, r)
        # a k block dropped from a sub-tile of panel 1 leaves no factor at all at this conditioning
        # (a later pivot turns negative): the GPU test sees that as fail = 1 where LAPACK succeeds
        G = C.restated_ll64(D2, pt, yv, fma=fma, mutant=C.FATAL_MUTANT)
        assert G is None or C.factor_check(G, D2, pt, yv)['ratio'] >= 100.0
    # one entry of an off-diagonal tile (panel 1, row tile 0) moved by 64 gamma_{n+1} of its scale
    for F in (good, C.lapack_factor(D2, pt, yv)[0]):
        for (i, j) in ((100, 70), (n - 1, 64), (n, 80)):
            r = C.factor_check(C.perturbed(F, i, j), D2, pt, yv)
            assert r['ratio'] > 1.0, (i, j, r)   # (the worst entry may be another one of row / column i)


def test_mean_reference_holds_the_double_evaluation():
    """The plain double evaluation of the posterior mean is inside the mean bound at every case,
    and a weight dropped from the sum is outside."""
    for n in C.MEAN_NS:
        for d in C.MEAN_DS:
            x, q, coef, alpha, bias = C.mean_case(n, d)
            assert np.abs(alpha).min() < 1e-2 and np.abs(alpha).max() > 1e9 or n == 1
            dist = C.dist_seq(x, q)
            for b in (None, bias):
                ref, bnd = C.mean_reference(x, q, coef, alpha, b)
                out = np.array([np.sum((coef[j, 1] * np.exp(coef[j, 0] * dist)) * alpha[j]) for j in range(d)])
                out = out + b if b is not None else out
                assert np.all(np.abs(out.astype(C.LD) - ref) <= bnd), (n, d)
                if n > 1:
                    k = int(np.argmax(np.abs(alpha[0])))
                    bad = out[0] - (coef[0, 1] * np.exp(coef[0, 0] * dist[k])) * alpha[0, k]
                    assert abs(C.LD(bad) - ref[0]) > bnd[0]


def test_d2_fallback_bound_holds_scipy():
    for d in C.DIM_DS:
        x, _, D2 = C.host_case(65, d)
        assert C.d2_fallback_ratio(D2, x) <= 1.0
