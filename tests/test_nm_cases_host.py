"""CPU checks behind tests/test_gpu_nm_matrix.py: that the tables of tests/nm_cases.py reach every
fit-side kernel instantiation, that the oracle which judges the kernels there is itself right at
those neighbour counts, and that the seeded inputs have the properties the GPU tests rely on.

-LML and posterior mean against 60-digit mpmath on the same double inputs, at the smallest and
largest m of every padded size and their neighbours, three thetas, jitters 1e-12 and 1e-16
(138 cases, cond2(K) from 1 to 7.7e10).  The error is scaled by eps * cond2(K) * max(1, |f|); the
yardstick is the reference's own formulation (models.py:86-91, 162-167, 240-244) in numpy/LAPACK,
and the oracle's largest scaled error may be at most twice numpy's and never has to be below 4: both
are backward-stable Choleskys that differ only in the order of their sums.  Measured here:
    -LML            oracle 4.70     numpy/LAPACK 3.85     (the oracle's at m = 25, theta (-1, -6), jitter 1e-12)
    posterior mean  oracle 0.00304  numpy/LAPACK 0.00277

With tolerance 1e9 a fit ends at its first check (nfev = 3) exactly when its three initial -LML
values lie within 1e9 of the smallest: |inf - x| and inf - inf are not <= fatol in scipy's rule
either, so a simplex with a +inf vertex goes on, and so does one on a kernel matrix so
ill-conditioned that -LML is ~1e10.  test_input_conditions pins that as an equivalence."""
import functools

import numpy as np
import pytest

import nm_cases as NC
import oracle as O

# ------------------------------------------------------------------------------------ coverage
_M6 = (8, 16, 18, 20, 24, 32)
_M8 = _M6 + (48, 64)
EXPECTED_INSTANTIATIONS = sorted(
    [('nm_spec_kernel', M) for M in _M8] +
    [('nm_spec2_kernel', M, W) for M in _M6 for W in (0, 2, 4)] +
    [('nm_fit_kernel', M, fused) for M in _M8 for fused in (False, True)] +
    [('gp_mean_kernel', M) for M in _M8] +
    [('gp_pre_kernel', M) for M in _M8] +
    [('chain_kernel', M) for M in (8, 16, 18, 20, 24)] +
    [('nm_lane_kernel', m, 4) for m in (10, 15)] +
    [('nm_lane1_kernel', m) for m in (10, 15)], key=str)


def test_tables_reach_every_instantiation():
    """Every (template, MAXM) of csrc/nngp_gp.hip and csrc/nngp_nmlane.hip, written out."""
    assert len(EXPECTED_INSTANTIATIONS) == 67
    assert sorted(NC.instantiations(), key=str) == EXPECTED_INSTANTIATIONS


def test_padded_sizes_restated():
    assert [NC.gp_mmin(M) for M in NC.MAXMS] == [1, 9, 17, 19, 21, 25, 33, 49]
    assert NC.EDGE_MS == [1, 8, 9, 16, 17, 18, 19, 20, 21, 24, 25, 32, 33, 48, 49, 64]
    for m in NC.ALL_MS:
        M = NC.maxm_for(m)
        assert NC.gp_mmin(M) <= m <= M and (M == 8 or m > NC.MAXMS[NC.MAXMS.index(M) - 1])
    assert [NC.k_image_doubles(M) for M in (8, 32, 48, 64)] == [8 * 9 + 32, 32 * 33 + 128, 24 * 49 + 192, 32 * 65 + 256]


@pytest.mark.parametrize('form', list(NC.FORMS))
def test_forced_forms_do_not_depend_on_the_cu_count(form):
    """Under a table entry's knobs expected_form never asks for the CU count (ncu = None raises
    where it would) and names the form's kernel, at every m the form accepts."""
    want = {'spec1': 'nm_spec_kernel', 'spec2w2': 'nm_spec2_kernel', 'spec2w4': 'nm_spec2_kernel',
            'fused': 'nm_fit_kernel', 'packed_queue': 'nm_fit_kernel', 'packed_static': 'nm_fit_kernel',
            'park_w4': 'nm_fit_kernel', 'park_w2': 'nm_fit_kernel', 'park_w1': 'nm_fit_kernel',
            'lanes4': 'nm_lane_kernel', 'lanes1': 'nm_lane1_kernel'}[form]
    for m in NC.ALL_MS:
        if not NC.form_accepts(form, m):
            continue
        nj, R = NC.form_shape(form, m)
        e = NC.expected_form(m, 3, nj, R, NC.FORMS[form])
        M = NC.maxm_for(m)
        assert e['kernels'][0][0] == want and e['kernels'][0][1] == (m if form.startswith('lanes') else M)
        if form == 'fused':
            # nine jitters: fused up to MAXM = 32; above, the coordinate's 144 threads exceed the
            # bound of 64 and the call falls through to the packed kernel and the mean kernel
            assert e['kernels'] == ([('nm_fit_kernel', M, True)] if m <= 32 else
                                    [('nm_fit_kernel', M, False), ('gp_mean_kernel', M)])
            assert e['cpw'] == (1 if m <= 32 else None)
        if form in ('packed_queue', 'packed_static'):
            assert e['mode'] == form[7:] and e['kernels'] == [('nm_fit_kernel', M, False), ('gp_mean_kernel', M)]
            assert form == 'packed_queue' or e['nblocks'] > 1   # (REFILL = 0 alone keeps the queue off)
        if form.startswith('park'):
            resume = {'park_w4': ('nm_spec2_kernel', M, 0), 'park_w2': ('nm_spec2_kernel', M, 0),
                      'park_w1': ('nm_spec_kernel', M)}[form]
            assert e['mode'] == 'park' and e['threads'] == 64 and e['kernels'][1] == resume
        if form.startswith('spec2'):
            assert e['kernels'][0][2] == int(form[-1])
    with pytest.raises(ValueError):
        NC.expected_form(20, 3, 9, 1, {})


def test_fused_edges():
    """thr(c) = roundup64(c * n_jitter * R * 16) against the launch bound 512 / 256 / 64."""
    F = NC.FORMS['fused']
    for m in NC.ALL_MS:
        M = NC.maxm_for(m)
        for (nj, R), fused in ((NC.fusing_shape(m), True), (NC.refusing_shape(m), False)):
            e = NC.expected_form(m, 3, nj, R, F)
            assert (e['mode'] == 'fused') == fused, (m, nj, R)
            if fused:
                assert e['threads'] == (nj * R * 16 + 63) // 64 * 64 <= NC.nm_tmax(M)
    assert NC.fusing_shape(16) == (9, 3) and NC.refusing_shape(16) == (9, 4)
    assert NC.fusing_shape(17) == (9, 1) and NC.refusing_shape(32) == (9, 2)
    assert NC.fusing_shape(33) == (4, 1) and NC.refusing_shape(64) == (5, 1)
    for m in NC.FUSED_D257_MS:   # two coordinates per workgroup, the last workgroup with one
        e = NC.expected_form(m, 257, 9, 1, F, ncu=NC.FUSED_D257_CUS)
        assert (e['mode'], e['cpw'], e['nblocks'], e['threads']) == ('fused', 2, 129, 320)


def test_batch_counts_fall_on_both_sides_of_the_launch_shapes():
    """n_fits against 4 fits per wave, 16 per workgroup and the queue's nblocks > 1."""
    q = lambda m, n: NC.expected_form(m, NC.BATCH_D, 9, 1, NC.FORMS['packed_queue'], api='fit_batch', n_fits=n)
    assert [q(16, n)['mode'] for n in (16, 17)] == ['static', 'queue']
    assert [q(64, n)['mode'] for n in (4, 5)] == ['static', 'queue']
    p = lambda n: NC.expected_form(16, NC.BATCH_D, 9, 1, NC.FORMS['park_w4'], api='fit_batch', n_fits=n)
    assert [p(n)['nblocks'] for n in (4, 5, 64, 65)] == [1, 2, 16, 17]


# -------------------------------------------------------------------- the oracle against mpmath
MP_MS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 18, 19, 20, 21, 24, 25, 31, 32, 33, 47, 48, 49, 63, 64)
MP_THETAS = ((-3.0, -4.0), (-1.0, -6.0), (-5.0, -2.0))
MP_JITTERS = (-12.0, -16.0)


def _mp_case(mp, D2, kd2, y, theta, jit, tol=None):
    """(-LML, posterior mean) at 60 digits from the double inputs.  tol: mpmath's absolute threshold
    of positive-definiteness (its default, 1e-60, refuses a kernel matrix of entries ~1e-160)."""
    m = len(y)
    sx, sy = mp.mpf(10) ** mp.mpf(theta[0]), mp.mpf(10) ** mp.mpf(theta[1])
    k = lambda r2: sy * mp.exp(-mp.mpf(r2) / (2 * sx))
    K = mp.matrix(m, m)
    for i in range(m):
        for j in range(i + 1):
            K[i, j] = K[j, i] = k(D2[i, j]) + (mp.mpf(jit) if i == j else 0)
    L = mp.cholesky(K, tol=tol)
    yv = [mp.mpf(v) for v in y]
    z = []
    for i in range(m):
        z.append((yv[i] - mp.fsum(L[i, j] * z[j] for j in range(i))) / L[i, i])
    alpha = [mp.mpf(0)] * m
    for i in reversed(range(m)):
        alpha[i] = (z[i] - mp.fsum(L[j, i] * alpha[j] for j in range(i + 1, m))) / L[i, i]
    f = (mp.fdot(yv, alpha) / 2 + mp.fsum(mp.log(L[i, i]) for i in range(m)) +
         mp.mpf(m) / 2 * mp.log(2 * mp.pi))
    mean = mp.fdot([k(v) for v in kd2], alpha)
    return f, mean


def _np_case(D2, kd2, y, theta, jit):
    """The reference's formulation in numpy/LAPACK: K + jitter*I, Cholesky, two triangular solves."""
    from scipy.linalg import solve_triangular
    m = len(y)
    k = lambda r2: 10 ** theta[1] * np.exp(-0.5 * (1 / (10 ** theta[0])) * r2)
    K = k(D2) + np.eye(m) * jit
    L = np.linalg.cholesky(K)
    alpha = solve_triangular(L.T, solve_triangular(L, y, lower=True), lower=False)
    f = -(-0.5 * y @ alpha - np.sum(np.log(np.diag(L))) - (m / 2) * np.log(2 * np.pi))
    return f, k(kd2) @ alpha, np.linalg.cond(K, 2)


@functools.lru_cache(maxsize=None)
def _mp_table():
    mp = pytest.importorskip('mpmath').mp
    mp.dps = 60
    eps = np.finfo(float).eps
    rows = []
    for m in MP_MS:
        xm, ym, q = NC.fit_case(m, 3, 'smooth')
        y = np.ascontiguousarray(ym[:, 0])
        D2 = O.d2_matrix(xm)
        kd2 = O.d2_matrix(np.vstack([xm, q]))[-1, :-1].copy()
        for theta in MP_THETAS:
            for je in MP_JITTERS:
                jit = float(10.0 ** je)
                f_mp, mean_mp = _mp_case(mp, D2, kd2, y, theta, jit)
                f_np, mean_np, cond = _np_case(D2, kd2, y, theta, jit)
                f_or, mean_or = O.nlml(D2, y, theta, je), O.gp_mean(xm, y, q, theta, je)
                assert np.isfinite([f_np, mean_np, f_or, mean_or]).all(), (m, theta, je)
                sc_f = eps * cond * max(1.0, abs(float(f_mp)))
                sc_m = eps * cond * max(1.0, abs(float(mean_mp)))
                rows.append((m, theta, je, cond,
                             float(abs(mp.mpf(f_or) - f_mp)) / sc_f, float(abs(mp.mpf(f_np) - f_mp)) / sc_f,
                             float(abs(mp.mpf(mean_or) - mean_mp)) / sc_m, float(abs(mp.mpf(mean_np) - mean_mp)) / sc_m))
    return rows


@pytest.mark.parametrize('what,col', [('nlml', 4), ('gp_mean', 6)])
def test_oracle_vs_mpmath_at_every_padded_edge(what, col):
    rows = _mp_table()
    assert len(rows) == 138
    conds = [r[3] for r in rows]
    e_or, e_np = max(r[col] for r in rows), max(r[col + 1] for r in rows)
    worst = max(rows, key=lambda r: r[col])
    print(f'{what}: largest err / (eps * cond2(K) * max(1, |f|)) over {len(rows)} cases, cond2(K) '
          f'{min(conds):.3g} .. {max(conds):.3g}: oracle {e_or:.3g} (m={worst[0]} theta={worst[1]} '
          f'jitter=1e{worst[2]:.0f}), numpy/LAPACK {e_np:.3g}')
    assert min(conds) < 10 and max(conds) > 1e10   # the table spans well- and ill-conditioned K
    assert e_or <= max(4.0, 2.0 * e_np)


# ------------------------------------------------------------------------ the 'scale' family
SCALE_MP_THETAS = (((-2.0, 150.6), -12.0), ((-3.0, 160.0), -20.0), ((-2.0, -151.0), -170.0), ((-3.0, -160.0), -170.0))


def test_scale_rows_reach_the_dispatch_table():
    """Every form at every scale m names kernels of the instantiation table, without the CU count:
    both lanes kernels at 10 and 15, the packed, one-level, two-level and resume kernels at the
    padded sizes 16 and 20, the packed and one-level ones at 48 and 64."""
    rows = NC.scale_rows()
    assert len(rows) == 11 + 11 + 9 + 5 + 5
    reached = set()
    for m, form in rows:
        e = NC.expected_form(m, NC.BATCH_D, len(NC.SCALE_JITTERS), 1, NC.FORMS[form], api='fit_batch',
                             n_fits=NC.SCALE_NFITS)
        assert e['rc'] == NC.NNGP_OK and set(e['kernels']) <= set(EXPECTED_INSTANTIATIONS), (m, form)
        reached.update(e['kernels'])
    want = ([('nm_lane_kernel', m, 4) for m in (10, 15)] + [('nm_lane1_kernel', m) for m in (10, 15)] +
            [('nm_fit_kernel', M, False) for M in (16, 20, 48, 64)] + [('nm_spec_kernel', M) for M in (16, 20, 48, 64)] +
            [('nm_spec2_kernel', M, W) for M in (16, 20) for W in (0, 2, 4)])
    assert sorted(reached, key=str) == sorted(want, key=str)
    # the packed forms split the list over more than one workgroup, the last wave is partial
    q = NC.expected_form(20, NC.BATCH_D, 3, 1, NC.FORMS['packed_static'], api='fit_batch', n_fits=NC.SCALE_NFITS)
    assert q['mode'] == 'static' and q['nblocks'] == 2 and NC.SCALE_NFITS % 4 != 0


def test_scale_case_conditions():
    """The conditions the 'scale' GPU tests rely on, from the oracle: adjacent fits differ in kind,
    every high or low matrix starts outside the set in_mid_range accepts (nm_cases checks that, and
    the crossing matrix at sy = 150.6, while it builds a case), every start and every result has a
    finite -LML, and the caps 3, 9, 11 end every fit there while 400 lets every fit converge."""
    assert NC.mid_accepts(2.0 ** -500) and not NC.mid_accepts(np.nextafter(2.0 ** -500, 0))
    assert NC.mid_accepts(np.nextafter(NC.MID_HI, 0)) and not NC.mid_accepts(NC.MID_HI) and NC.mid_accepts(2.0 ** 500)
    for m in NC.SCALE_MS:
        xm, ym, coord, jidx, th0, kind = NC.scale_fit_case(m)
        assert all(kind[i] != kind[i + 1] for i in range(len(kind) - 1))
        assert all({'ord', 'high', 'low'} == set(kind[w:w + 4]) for w in range(0, len(kind) - 3, 4))
        high, low = [k == 'high' for k in kind], [k == 'low' for k in kind]
        assert set(th0[high, 1]) == set(NC.SCALE_HIGH_SY) and set(th0[low, 1]) == set(NC.SCALE_LOW_SY)
        assert set(th0[:, 0]) == set(NC.SCALE_SX) and np.all(NC.SCALE_JITTERS[jidx[low]] == -170.0)
        for tol, maxfev in NC.SCALE_SETTINGS:
            theta, fval, nfev = NC.scale_fit_oracle(m, tol, maxfev)
            assert np.isfinite(fval).all() and np.isfinite(theta).all()
            assert np.all(nfev == maxfev) if maxfev < 400 else np.all(nfev < 400)
        # at the cap of 3 the high and low fits still sit at their out-of-range starts
        theta3 = NC.scale_fit_oracle(m, 0.1, 3)[0]
        assert np.all(theta3[high, 1] > 150.5) and np.all(theta3[low, 1] < -150.9)
    for M in NC.MAXMS:
        *_, want, kind = NC.scale_mean_case(M)
        assert np.isfinite(want).all() and len(set(kind)) == 3


@functools.lru_cache(maxsize=None)
def _mp_scale_table():
    mp = pytest.importorskip('mpmath').mp
    mp.dps = 60
    eps = np.finfo(float).eps
    rows = []
    for m in NC.SCALE_MS:
        xm, ym, q = NC.fit_case(m, NC.BATCH_D, 'smooth')
        y = np.ascontiguousarray(ym[:, 0])
        D2 = O.d2_matrix(xm)
        kd2 = O.d2_matrix(np.vstack([xm, q]))[-1, :-1].copy()
        for theta, je in SCALE_MP_THETAS:
            jit = float(10.0 ** je)
            f_mp, mean_mp = _mp_case(mp, D2, kd2, y, theta, jit, tol=mp.mpf(0))
            f_np, mean_np, cond = _np_case(D2, kd2, y, theta, jit)
            f_or, mean_or = O.nlml(D2, y, theta, je), O.gp_mean(xm, y, q, theta, je)
            assert np.isfinite([f_np, mean_np, f_or, mean_or]).all(), (m, theta, je)
            sc_f = eps * cond * max(1.0, abs(float(f_mp)))
            sc_m = eps * cond * max(1.0, abs(float(mean_mp)))
            rows.append((m, theta, je, cond,
                         float(abs(mp.mpf(f_or) - f_mp)) / sc_f, float(abs(mp.mpf(f_np) - f_mp)) / sc_f,
                         float(abs(mp.mpf(mean_or) - mean_mp)) / sc_m, float(abs(mp.mpf(mean_np) - mean_mp)) / sc_m))
    return rows


@pytest.mark.parametrize('what,col', [('nlml', 4), ('gp_mean', 6)])
def test_oracle_vs_mpmath_scale_rows(what, col):
    """The oracle that judges the 'scale' rows, at their signal variances 10^150.6, 10^160, 10^-151
    and 10^-160 (jitter 1e-170 under the low ones): the same yardstick and bound as above."""
    rows = _mp_scale_table()
    assert len(rows) == 20
    e_or, e_np = max(r[col] for r in rows), max(r[col + 1] for r in rows)
    worst = max(rows, key=lambda r: r[col])
    print(f'{what}, scale rows: largest err / (eps * cond2(K) * max(1, |f|)) over {len(rows)} cases: oracle '
          f'{e_or:.3g} (m={worst[0]} theta={worst[1]} jitter=1e{worst[2]:.0f}), numpy/LAPACK {e_np:.3g}')
    assert e_or <= max(4.0, 2.0 * e_np)


# ------------------------------------------------------------------- conditions on the inputs
def _first_check_ends(m, variant, tol, n_jitter=9, R=1, d=3):
    """Per fit of a prediction case: does scipy's rule end it at the first check, i.e. do the three
    -LML values of the initial simplex (x0, and x0 with one component times 1.05, or 0.00025 where
    it is zero), by the oracle, lie within tol of the smallest?  (inf - inf and |inf - x| do not.)"""
    X, Y, q, th0 = NC.predict_case(m, variant, d, n_jitter, R)
    idx, _ = O.knn(X, q, m)
    D2 = O.d2_matrix(X[idx])
    jit = NC.jitters_for(n_jitter)
    out = []
    for f in range(len(th0)):
        c, a = f // (n_jitter * R), (f // R) % n_jitter
        y = np.ascontiguousarray(Y[idx, c])
        fs = []
        for k in (None, 0, 1):
            th = th0[f].copy()
            if k is not None:
                th[k] = 1.05 * th[k] if th[k] != 0 else 0.00025
            fs.append(O.nlml(D2, y, th, jit[a]))
        fs = np.sort(fs)
        with np.errstate(invalid='ignore'):
            out.append(bool(np.max(np.abs(fs[0] - fs[1:])) <= tol))
    return np.array(out)


def test_input_conditions():
    n400 = ninf = total = 0
    for m in range(2, 65):
        fits = NC.oracle_predict(m, 'dup', 3, 9, 1, 0.1, 0.1, 400)[1]
        n400 += int((fits[:, 3] >= 400).sum())
        ninf += int(np.isinf(fits[:, 2]).sum())
        total += len(fits)
    print(f"'dup', m = 2..64: {n400} of {total} fits reach maxfev = 400, {ninf} end at +inf")
    assert total == 1701 and n400 >= 40 and ninf >= 1
    n3 = nlong = 0
    for m in NC.EDGE_MS:
        for variant in ('dup', 'zero'):
            fits = NC.oracle_predict(m, variant, 3, 9, 1, 0.0, 0.0, 60)[1]
            assert np.all(fits[:, 3] == 60), (m, variant)
            fits = NC.oracle_predict(m, variant, 3, 9, 1, 1e9, 1e9, 400)[1]
            ends = _first_check_ends(m, variant, 1e9)
            assert np.array_equal(fits[:, 3] == 3, ends), (m, variant)
            n3 += int(ends.sum())
            nlong += int((~ends).sum())
    print(f'tolerance 1e9: {n3} fits end at nfev = 3, {nlong} start with a +inf vertex or a spread above 1e9 and go on')
    assert n3 >= 600 and nlong >= 20
    theta0 = NC.predict_case(9, 'zero')[3]
    assert (theta0[:, 0] == 0).sum() >= 13 and (theta0[:, 1] == 0).sum() >= 9 and (theta0 == 0).all(axis=1).any()


def test_mean_case_has_a_failing_cholesky():
    """The theta tests/test_gpu_nm_matrix.py adds to every nngp_gp_mean case gives NaN on 'dup'."""
    for m in (3, 4, 16, 17, 33, 64):
        xm, ym, q = NC.fit_case(m, 3, 'dup')
        assert np.isnan(O.gp_mean(xm, ym[:, 0], q, NC.SINGULAR_THETA, NC.JITTERS[0]))
        assert np.isfinite(O.gp_mean(xm, ym[:, 0], q, (-5.0, -2.0), NC.JITTERS[-1]))


def test_fit_list_is_not_in_product_order():
    coord, jidx, th0 = NC.fit_list(65, NC.BATCH_D, 9, 7)
    assert len(set(zip(coord.tolist(), jidx.tolist()))) < 65            # repeats
    assert np.any(np.diff(coord) < 0) and np.any(np.diff(jidx) < 0)     # shuffled
    assert coord.dtype == np.int32 and jidx.dtype == np.int32 and th0.shape == (65, 2)
    assert set(coord.tolist()) == set(range(NC.BATCH_D)) and jidx.max() == 8
