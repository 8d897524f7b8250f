"""GPU: every form of the ELM kernels (csrc/nngp_elm.hip) at its dispatch edges, bit for bit against
the NumPy restatement of the arithmetic contract (tests/elm_ref.py).  No tolerance
anywhere: every comparison is array_equal on bit patterns.  The restatement is tied to the reference's
ELM_base at these widths on the CPU (tests/test_elm_host.py, tests/golden/elm_wide.npz).

What selects a form (hidden_launch, nngp_elm_hidden, elm_solve_kernel):
  d <= 2048            elm_hidden_kernel<4> (four rows per tile, 64 KB of LDS at d = 2048), else <1>;
  nch = ceil(n_poly / ELM_CHUNK)   the combine kernels add nch chunk sums; the wave form loads 64 at a time;
  rows * res <= 4096   elm_combine_wave_kernel, else elm_combine_kernel;
  few workgroups       the hidden units split over gridDim.y in groups of 4 (tails at res % 4 != 0);
  rows > max_rows      batches through the 64 MB partial-sum scratch;
  res > 64             more than one trip of every lane loop of elm_solve_kernel.
"""
import glob
import os
import re

import numpy as np
import pytest

import elm_ref as E
from conftest import ROOT
from elm_cases import EPS, RUNS, run_cfg
from test_gpu_elm import _bits, _dev, _gpu_predict, _lorenz, _ref_predict, _same

pytestmark = pytest.mark.gpu


def _header_int(name):
    src = open(glob.glob(os.path.join(ROOT, '*', 'csrc', 'nngp_elm.h'))[0]).read()
    return int(re.search(r'constexpr int %s = (\d+);' % name, src).group(1))


def _nch(d, deg):
    return -(-E.n_poly(d, deg) // E.CHUNK)


def _hidden_case(gpu, d, deg, res, rows_list, seed):
    """The model, its device rows and the restatement's hidden rows of max(rows_list) seeded rows."""
    X = np.random.default_rng(seed).uniform(-1, 1, (max(rows_list), d))
    mdl = gpu.ELM_base(d=d, res_size=res, degree=deg)
    bias, C = E.draw_weights(d, 47, res, deg)
    ref = E.hidden(X, bias, C, deg)
    return mdl, _dev(X), ref


def _relu_matters(ref):
    """Both branches of the relu; a result of few elements must at least hold a sum (a 0 hides it)."""
    assert np.any(ref > 0)
    if ref.size > 8:
        assert np.any(ref == 0)


# ------------------------------------------------------------------------------ nngp_elm_hidden
# one chunk (n_poly = 10).  A single row or tile: gridDim.y = ceil(res / 4) = 17, 125, 256, 256 groups
# of 4 hidden units, the last group partial at res 65 and 1023; 5 rows: two tiles, the second of one
# row; 70 rows: 18 tiles, gridDim.y = 114, so at res 500 and up a wave takes a second and a third unit.
# rows * res at res 1024: 4 * 1024 = 4096 is the wave combine's last size, 5 * 1024 the block combine's first.
@pytest.mark.parametrize('res', [65, 500, 1023, 1024])
def test_hidden_unit_tails_and_the_combine_switch(gpu, res):
    rows_list = (1, 4, 5, 70)
    mdl, Xd, ref = _hidden_case(gpu, 3, 2, res, rows_list, 300 + res)
    _relu_matters(ref)
    _relu_matters(ref[:1])
    for rows in rows_list:
        got = mdl.hidden_device(Xd[:rows]).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(ref[:rows])), rows
    if res == 1024:
        assert 4 * res == 4096 < 5 * res


# nch = 64: the wave combine's single full load block; 65: one chunk in its second block; 129: a third
# block of one chunk.  rows * res <= 24: the wave combine.
@pytest.mark.parametrize('d,nch,rows_list', [(360, 64, (1, 6)), (361, 65, (1, 6)), (512, 129, (5,))])
def test_many_chunks_through_the_wave_combine(gpu, d, nch, rows_list):
    assert _nch(d, 2) == nch
    mdl, Xd, ref = _hidden_case(gpu, d, 2, 4, rows_list, 400 + d)
    _relu_matters(ref)
    _relu_matters(ref[:1])
    for rows in rows_list:
        assert rows * 4 <= 4096
        got = mdl.hidden_device(Xd[:rows]).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(ref[:rows])), rows


def test_many_chunks_through_the_block_combine(gpu):
    """d = 512 at res_size 4 reaches only the wave combine (5 * 4 <= 4096), so res_size 1024 is added:
    5 * 1024 > 4096, elm_combine_kernel over nch = 129.  C is 1024 x 131 841 (1.08 GB), so the
    restatement is run on 16 of the hidden units (a unit's bits depend on its own row of C alone: the
    first and last groups of 4, the units around 511) and every unit is covered by the five rows taken
    one at a time, 1024 elements each, which the wave combine adds.  The weights are the model's own
    (a second draw of 135e6 numbers is a second; every other case here draws them independently)."""
    d, res, rows = 512, 1024, 5
    assert _nch(d, 2) == 129 and rows * res > 4096 >= res
    X = np.random.default_rng(912).uniform(-1, 1, (rows, d))
    mdl = gpu.ELM_base(d=d, res_size=res)
    Xd = _dev(X)
    got = mdl.hidden_device(Xd).cpu().numpy()
    units = np.r_[0:4, 509:517, 1020:1024]
    ref = E.hidden(X, mdl.bias[units, 0], mdl.R * mdl.C[units], 2)
    _relu_matters(ref)
    assert np.array_equal(_bits(got[:, units]), _bits(ref))
    single = np.vstack([mdl.hidden_device(Xd[r:r + 1]).cpu().numpy() for r in range(rows)])
    _relu_matters(single)
    assert np.array_equal(_bits(got), _bits(single))


# d = 2048: elm_hidden_kernel<4> with 4 * 2048 doubles = exactly 64 KB of dynamic LDS, 5 rows = a tile
# and a tail of one; d = 2049: elm_hidden_kernel<1>, 3 tiles of one row.  Degree 1 is 3 chunks, degree 2
# 2 052 / 2 054 chunks.
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('d,rows', [(2048, 5), (2049, 3)])
def test_row_tile_forms_at_the_lds_edge(gpu, d, rows, deg):
    assert 4 * 2048 * 8 == 64 << 10
    mdl, Xd, ref = _hidden_case(gpu, d, deg, 2, (rows,), 500 + d + deg)
    _relu_matters(ref)
    got = mdl.hidden_device(Xd).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(ref))


# the largest d: degree 1 (9 chunks, the last of one feature), and degree 2 with the largest n_poly
# (33 566 721 features, 32 781 chunks): the pair (i, j) closed form and its fix-up up to the last
# pair (8191, 8191).  One hidden unit and one row there: the seed is one whose sum is positive.
@pytest.mark.parametrize('deg,res,rows,seed', [(1, 5, 2, 601), (2, 1, 1, 602)])
def test_largest_d(gpu, deg, res, rows, seed):
    d = 8192
    mdl, Xd, ref = _hidden_case(gpu, d, deg, res, (rows,), seed)
    _relu_matters(ref)
    got = mdl.hidden_device(Xd).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(ref))


def test_rows_in_batches_through_the_partial_sum_scratch(gpu):
    d, res, rows = 128, 1024, 911
    chunk, tile = _header_int('ELM_CHUNK'), _header_int('ELM_ROW_TILE')
    assert chunk == E.CHUNK
    nch = -(-E.n_poly(d, 2) // chunk)
    max_rows = (64 << 20) // (8 * nch * res) // tile * tile   # nngp_elm_hidden
    assert (nch, max_rows) == (9, 908) and rows > max_rows
    X = np.random.default_rng(128).uniform(-1, 1, (rows, d))
    mdl = gpu.ELM_base(d=d, res_size=res)
    bias, C = E.draw_weights(d, 47, res, 2)
    Xd = _dev(X)
    got = mdl.hidden_device(Xd).cpu().numpy()
    pick = np.r_[0, 3, 455, 904:911]   # both batches, the first batch's last tile, the second's only one
    ref = E.hidden(X[pick], bias, C, 2)
    _relu_matters(ref)
    assert np.array_equal(_bits(got[pick]), _bits(ref))
    two = np.vstack([mdl.hidden_device(Xd[:max_rows]).cpu().numpy(), mdl.hidden_device(Xd[max_rows:]).cpu().numpy()])
    assert np.array_equal(_bits(got), _bits(two))
    assert np.array_equal(_bits(got[905:]), _bits(mdl.hidden_device(Xd[905:]).cpu().numpy()))


# ----------------------------------------------------------------------------- nngp_elm_predict
def _check_prediction(gpu, X, Y, q, ug, ref, **kw):
    """With bias / out and preds, with bias / out alone (inside _gpu_predict) and bare."""
    mdl = gpu.ELM_base(d=X.shape[1], **kw)
    preds, out = _gpu_predict(mdl, X, Y, q, ug)
    assert np.array_equal(_bits(preds), _bits(ref)), kw
    assert np.array_equal(_bits(out), _bits(ref + ug)), kw
    bare, _ = _gpu_predict(mdl, X, Y, q)
    assert np.array_equal(_bits(bare), _bits(ref)), kw
    return mdl


# res 64: one full trip of the lane loops; 65: a second trip of one lane; 128: two full trips; 500: the
# reference's default width; 1024: the LDS arrays full.  d = 70: a full and a partial coordinate
# block of the d-long pass.  m = 16 fills cm / gl / Qw.
@pytest.mark.parametrize('res,deg', [(64, 2), (65, 2), (128, 2), (500, 2), (1024, 2), (500, 1), (65, 1)])
def test_wide_predictions_are_bitwise_the_restatement(gpu, res, deg):
    for d in (3, 70):
        rng = np.random.default_rng(1000 * deg + 10 * res + d)
        bias, C = E.draw_weights(d, 47, res, deg)
        Xall, Yall = rng.uniform(-1, 1, (40, d)), rng.uniform(-1, 1, (40, d))
        q, ug = rng.uniform(-1, 1, d), rng.uniform(-1, 1, d)
        for m in (2, 5, 16):
            for rows in (40, m):
                X, Y = Xall[:rows], Yall[:rows]
                ref = _ref_predict(X, Y, q, m, bias, C, deg)
                assert np.all(np.isfinite(ref))
                _check_prediction(gpu, X, Y, q, ug, ref, res_size=res, m=m, degree=deg)


@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('res', [1, 2, 3])
def test_more_neighbours_than_hidden_units(gpu, res, deg):
    d, m = 3, 16
    rng = np.random.default_rng(70 + 10 * res + deg)
    bias, C = E.draw_weights(d, 47, res, deg)
    X, Y = rng.uniform(-1, 1, (40, d)), rng.uniform(-1, 1, (40, d))
    q, ug = rng.uniform(-1, 1, d), rng.uniform(-1, 1, d)
    idx = E.knn(X, q, m)
    Hn = E.hidden(X[idx], bias, C, deg)
    ref, kept = E.solve(Hn, Y[idx], E.hidden(q, bias, C, deg)[0], return_kept=True)
    assert len(kept) <= res < m - 1 and np.all(np.isfinite(ref))   # the threshold drops rows, not only duplicates
    assert len(kept) >= 1 and np.unique(Hn, axis=0).shape[0] > res + 1   # and not because the rows coincide
    _check_prediction(gpu, X, Y, q, ug, ref, res_size=res, m=m, degree=deg)


@pytest.mark.parametrize('res,m', [(20, 5), (500, 16)])
def test_dead_relu_predicts_the_nearest_target(gpu, res, m):
    import torch
    d = 3
    rng = np.random.default_rng(80 + res)
    X, Y = rng.uniform(-1, 1, (40, d)), rng.uniform(-1, 1, (40, d))
    q, ug = rng.uniform(-1, 1, d), rng.uniform(-1, 1, d)
    mdl = gpu.ELM_base(d=d, res_size=res, m=m)
    mdl.bias[:] = -1e3   # before the first device use: |C . phi| <= n_poly = 10, every pre-activation is negative
    bias, C = E.draw_weights(d, 47, res, 2)
    bias[:] = -1e3
    assert not np.any(E.hidden(X, bias, C, 2)) and not np.any(E.hidden(q, bias, C, 2))
    nearest = E.knn(X, q, m)[0]
    ref = _ref_predict(X, Y, q, m, bias, C)
    assert np.array_equal(_bits(ref), _bits(Y[nearest]))   # 0 > TAU * 0 is false: no row is kept
    preds, out = _gpu_predict(mdl, X, Y, q, ug)
    assert not torch.any(mdl.device_state()[2][:40]).item()
    assert np.array_equal(_bits(preds), _bits(Y[nearest]))
    assert np.array_equal(_bits(out), _bits(Y[nearest] + ug))
    bare, _ = _gpu_predict(mdl, X, Y, q)
    assert np.array_equal(_bits(bare), _bits(Y[nearest]))


def test_wide_prediction_on_a_large_training_set(gpu):
    """fit() of 5 000 rows at res_size 500: the neighbours' hidden rows come out of elm_combine_kernel
    (one batch: max_rows = 16 776).  Besides the prediction, a sample of the cached rows (the first and
    last tiles and 48 seeded ones) is held to the restatement."""
    d, res, m, rows = 3, 500, 16, 5000
    rng = np.random.default_rng(5000)
    bias, C = E.draw_weights(d, 47, res, 2)
    X, Y = rng.uniform(-1, 1, (rows, d)), rng.uniform(-1, 1, (rows, d))
    q, ug = rng.uniform(-1, 1, d), rng.uniform(-1, 1, d)
    ref = _ref_predict(X, Y, q, m, bias, C)
    assert np.all(np.isfinite(ref)) and rows * res > 4096
    mdl = _check_prediction(gpu, X, Y, q, ug, ref, res_size=res, m=m)
    pick = np.unique(np.r_[0:8, rows - 8:rows, rng.integers(0, rows, 48)])
    Hd = mdl.device_state()[2]
    refH = E.hidden(X[pick], bias, C, 2)
    _relu_matters(refH)
    assert np.array_equal(_bits(Hd[:rows].cpu().numpy()[pick]), _bits(refH))


# -------------------------------------------------------------------------- ELM_base.fit_device
def test_device_cache_grows_appends_and_resets(gpu):
    """40 rows (a buffer of 64), 64 (it fits), 65 (doubled to 128, the 64 cached rows copied), 200
    (to 256), then 30 (fewer rows than cached: computed afresh)."""
    d, res, m = 3, 65, 5
    rng = np.random.default_rng(9)
    bias, C = E.draw_weights(d, 47, res, 2)
    X, Y = rng.uniform(-1, 1, (200, d)), rng.uniform(-1, 1, (200, d))
    q = rng.uniform(-1, 1, d)
    refH = E.hidden(X, bias, C, 2)
    _relu_matters(refH)
    Xd, Yd, qd = _dev(X), _dev(Y), _dev(q)
    mdl = gpu.ELM_base(d=d, res_size=res, m=m)
    caps = []
    for k, rows in enumerate((40, 64, 65, 200, 30)):
        mdl.fit(Xd[:rows], Yd[:rows], k)
        Xs, Ys, H, n = mdl.device_state()
        assert n == rows and H.shape[0] >= rows and H.shape[1] == res
        caps.append(H.shape[0])
        assert np.array_equal(_bits(H[:rows].cpu().numpy()), _bits(refH[:rows])), rows
        ref = _ref_predict(X[:rows], Y[:rows], q, m, bias, C)
        assert np.all(np.isfinite(ref))
        assert np.array_equal(_bits(mdl.predict_device(qd).cpu().numpy()), _bits(ref)), rows
    assert caps == [64, 64, 128, 256, 64]
    # appended rows only: rows the cache holds are not computed again
    mdl.fit(Xd[:40], Yd[:40], 0)
    H = mdl.device_state()[2]
    H[:40] = -1.0
    mdl.fit(Xd[:64], Yd[:64], 1)
    H2 = mdl.device_state()[2].cpu().numpy()
    assert np.all(H2[:40] == -1.0) and np.array_equal(_bits(H2[40:64]), _bits(refH[40:64]))


# ----------------------------------------------------------------- the driver and the native sweep
@pytest.mark.parametrize('kw', [dict(res_size=500, m=5, degree=2), dict(res_size=100, m=16, degree=1)],
                         ids=['res500_m5_deg2', 'res100_m16_deg1'])
def test_wide_and_degree_1_runs_are_bitwise_the_restatement_loop(gpu, monkeypatch, kw):
    assert RUNS['lorenz'][2] == 32
    so, u0, args = run_cfg('lorenz')
    o = E.parareal_elm(so, *args, epsilon=EPS, u0=u0, early_stop=3, **kw)
    assert o['k'] == 3 and o['conv_int'] == [1, 2, 3]   # three full sweeps, on the restatement
    assert not np.any(np.isnan(o['u'])) and not np.any(np.isnan(o['err']))
    native = _lorenz(gpu)[2].run(model='elm', early_stop=3, **kw)
    assert native['k'] == 3 and native['conv_int'] == o['conv_int']
    assert _same(native['u'], o['u']) and _same(native['err'], o['err'])
    ode, s, p = _lorenz(gpu)
    monkeypatch.setattr(s, 'coarse_is_paged', lambda: True)   # the driver's per-slice Python sweep
    per_slice = p.run(model='elm', early_stop=3, **kw)
    assert per_slice['k'] == 3 and per_slice['conv_int'] == o['conv_int']
    assert _same(per_slice['u'], o['u']) and _same(per_slice['err'], o['err'])
