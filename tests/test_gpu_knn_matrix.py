"""The kNN select and the neighbour geometry pinned to the oracle at every form, bitwise.

The correction's first kernel (csrc/nngp_gp.hip knn_select_dev, launch_knn_select) has five
instantiations by ceil(rows/256) -- register keys K = 2, 4, 8, 16, streaming K = 0 with or without
the LDS key cache -- and two algorithms in each: the radix threshold select while at most
SEL_CAND = 256 rows have a key whose high word is at or below the m-th smallest, the m-round
fallback otherwise.  tests/knn_cases.py builds the inputs that reach each of them at its dispatch
edges (tests/test_knn_cases_host.py checks, on the CPU, that they do); here

* nngp_knn's idx_out / dist_out against numpy's stable argsort (knn_cases.ref_knn) and the
  oracle: the edges 512/513 ... 14336/14337, m = 1 and m = rows, exact ties on both sides of 256
  candidates (the K > 0 rounds: per-thread sort, head pop, exhausted 16-lane rows, rank merges),
  keys that differ in the low word only, NaN / +inf / subnormal / zero distances, and both branches
  of knn_dist_row (double2 blocks of 32 columns on 16-byte aligned rows, scalar otherwise);
* nngp_predict -- fits, preds and preds + bias -- against oracle.predict through every geometry
  form after the select (sequential d < 8, the octet form 8 <= d <= 128, a wave or a thread per
  pair for d > 128 or unstaged rows) on each side of its switches, and through the key-staged
  selects whose staged neighbour rows reuse the same dynamic LDS;
* nngp_correction_sweep called directly on a synthetic training set: the batched select
  (blockIdx.y = guessed query) and the hit check, against the oracle's loop and its predicted hits.

No tolerance anywhere: the same operations in the same order on both sides."""
import ctypes

import numpy as np
import pytest

import knn_cases as KC
import oracle as O

pytestmark = pytest.mark.gpu


def _t(torch, a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device='cuda')


def _offset(torch, a, off):
    """Device copy of `a`; off: a view starting one double into a larger buffer (torch's
    allocations are at least 256-byte aligned, so the view is 8-byte aligned only)."""
    if not off:
        t = _t(torch, a)
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(a.size + 1, dtype=torch.float64, device='cuda')
    v = buf[1:].view(a.shape)
    v.copy_(_t(torch, a))
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


def _knn(gpu, torch, X, q, m, want_dist=True, offset=None):
    rows, d = X.shape
    Xt = _offset(torch, X, offset == 'X')
    qt = _offset(torch, q, offset == 'q')
    idx = torch.full((m,), -7, dtype=torch.int32, device='cuda')
    dist = torch.full((m,), -7.0, dtype=torch.float64, device='cuda') if want_dist else None
    gpu._lib.check(gpu.lib().nngp_knn(Xt.data_ptr(), rows, d, qt.data_ptr(), m, idx.data_ptr(),
                                      dist.data_ptr() if want_dist else None, None))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy() if want_dist else None


# ----------------------------------------------------------------------------------- nngp_knn
_KEY_LDS_CASES = [c for c in KC.CASES if KC.case_rows(c) > 4096]


def _check_knn_case(gpu, case):
    import torch
    X, q = KC.build(case)
    m = case['m']
    gi, gd = _knn(gpu, torch, X, q, m, offset=case.get('offset'))
    ri, rd, _ = KC.ref_knn(X, q, m)
    oi, od = O.knn(X, q, m)
    assert np.array_equal(gi, ri), (gi, ri)
    assert np.array_equal(gd, rd, equal_nan=True)
    assert np.array_equal(gi, oi) and np.array_equal(gd, od, equal_nan=True)


@pytest.mark.parametrize('case', KC.CASES, ids=KC.CASE_IDS)
def test_knn_case_vs_numpy_and_oracle(gpu, case):
    _check_knn_case(gpu, case)


@pytest.mark.parametrize('case', _KEY_LDS_CASES, ids=[c['id'] for c in _KEY_LDS_CASES])
def test_knn_case_without_key_cache(gpu, case, monkeypatch):
    """rows > 4 096 again with NNGP_KEY_LDS=0: the streaming select re-reading its keys from memory
    (the default stages them in LDS up to 14 336 rows; 14 337 streams either way)."""
    monkeypatch.setenv('NNGP_KEY_LDS', '0')
    _check_knn_case(gpu, case)


def _select_forms():
    """One case per (instantiation, algorithm), the streaming ones with and without the cache."""
    form = lambda rows: next((k for k in (2, 4, 8, 16) if rows <= 256 * k), 0)
    seen, out = set(), []
    for c in KC.CASES:
        key = (form(KC.case_rows(c)), c['side'])
        if c['side'] and c['kind'] in ('tie', 'low') and key not in seen:
            seen.add(key)
            out += [(c, None)] + ([(c, '0')] if key[0] == 0 else [])
    return out


@pytest.mark.parametrize('case,key_lds', _select_forms(),
                         ids=[c['id'] + ('-nocache' if k else '') for c, k in _select_forms()])
def test_knn_without_dist_out(gpu, case, key_lds, monkeypatch):
    import torch
    if key_lds is not None:
        monkeypatch.setenv('NNGP_KEY_LDS', key_lds)
    X, q = KC.build(case)
    gi, _ = _knn(gpu, torch, X, q, case['m'], want_dist=False)
    assert np.array_equal(gi, KC.ref_knn(X, q, case['m'])[0])


@pytest.mark.parametrize('rows,d,m', [(50, 3, 0), (100, 3, 65), (20, 3, 21), (50, 0, 5)])
def test_knn_refusals_launch_nothing(gpu, rows, d, m):
    import torch
    X = _t(torch, np.ones((rows, max(d, 1))))
    q = _t(torch, np.zeros(max(d, 1)))
    idx = torch.full((70,), -7, dtype=torch.int32, device='cuda')
    dist = torch.full((70,), -7.0, dtype=torch.float64, device='cuda')
    with pytest.raises(gpu._lib.NNGPError):
        gpu._lib.check(gpu.lib().nngp_knn(X.data_ptr(), rows, d, q.data_ptr(), m, idx.data_ptr(), dist.data_ptr(), None))
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((dist == -7.0).all())


# ------------------------------------------------------------------------------- nngp_predict
_PREDICT_ORACLE = {}


def _predict_variants():
    out = []
    for s in KC.PREDICT_SHAPES:
        for key_lds in ([None, '0'] if s[2] > 4096 else [None]):
            for waves in (None, '0'):
                out.append((s, waves, key_lds))
    return out


def _variant_id(v):
    s, waves, key_lds = v
    return KC.predict_id(s) + ('-pairs' if waves else '') + ('-nocache' if key_lds else '')


@pytest.mark.parametrize('variant', _predict_variants(), ids=_variant_id)
def test_predict_select_and_geometry_forms_vs_oracle(gpu, variant, monkeypatch):
    """fits_out, preds and out = preds + bias of nngp_predict bitwise the oracle's predict, with
    NNGP_D2_WAVES unset and 0 (a thread per pair instead of a wave where the select itself does not
    compute D2) and, above 4 096 rows, NNGP_KEY_LDS=0 too."""
    import torch
    shape, waves, key_lds = variant
    m, d, rows = shape[:3]
    if waves is not None:
        monkeypatch.setenv('NNGP_D2_WAVES', waves)
    if key_lds is not None:
        monkeypatch.setenv('NNGP_KEY_LDS', key_lds)
    X, Y, q = KC.predict_data(shape)
    mdl = gpu.NNGP_p(n=d, N=4, nn=m, seed=3)
    th0 = mdl.draw_thetas(1)
    if shape not in _PREDICT_ORACLE:
        _PREDICT_ORACLE[shape] = O.predict(X, Y, q, m, th0, return_fits=True)
    ora, ofits = _PREDICT_ORACLE[shape]
    bias = np.random.default_rng(d).standard_normal(d)
    fits = torch.full((mdl.n_fits, 4), -7.0, dtype=torch.float64, device='cuda')
    out = torch.full((d,), -7.0, dtype=torch.float64, device='cuda')
    preds = mdl.predict_device(_t(torch, X), _t(torch, Y), rows, _t(torch, q), _t(torch, th0), fits_out=fits,
                               out=out, bias=_t(torch, bias)).cpu().numpy()
    assert np.array_equal(fits.cpu().numpy(), ofits, equal_nan=True)
    assert np.array_equal(preds, ora, equal_nan=True)
    assert np.array_equal(out.cpu().numpy(), ora + bias, equal_nan=True)


# ---------------------------------------------------------------------- nngp_correction_sweep
_SWEEP_FIRST = {}


def _sweep(gpu, S, speculate):
    """nngp_correction_sweep over the whole case (I = 0): (U1, UG1, spec_hits)."""
    import torch
    ode = gpu.Lorenz(normalization='-11')
    solver = gpu.SolverRK(ode.get_vector_field(), Ng=KC.SWEEP_NG, Nf=KC.SWEEP_NF, F='RK4', G='RK1')
    dev = torch.device('cuda', torch.cuda.current_device())
    cs = solver.f.csystem(dev)
    N, m, d = S['N'], S['m'], 3
    t = _t(torch, S['t'])
    U1 = torch.full((N + 1, d), -7.0, dtype=torch.float64, device='cuda')
    UG1 = torch.full((N + 1, d), -7.0, dtype=torch.float64, device='cuda')
    U1[0] = _t(torch, S['U1'][0])
    UF, UG, X, Y, th0 = (_t(torch, S[k]) for k in ('UF', 'UG', 'X', 'Y', 'th0'))
    scratch = torch.empty(d, dtype=torch.float64, device='cuda')
    jit, jp = gpu._lib.host_doubles(O.JITTERS)
    hits = ctypes.c_int32(-1)
    gpu._lib.check(gpu.lib().nngp_correction_sweep(
        ctypes.byref(cs), gpu._lib.TABLEAU['RK1'], solver.step_mode, KC.SWEEP_NG, t.data_ptr(), 0, N, U1.data_ptr(),
        UG1.data_ptr(), UF.data_ptr(), UG.data_ptr(), gpu._lib.MODEL_NNGP, X.data_ptr(), Y.data_ptr(), S['rows'], m,
        len(jit), jp, 1, th0.data_ptr(), 0.1, 0.1, 400, scratch.data_ptr(), speculate, ctypes.byref(hits), None,
        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return U1.cpu().numpy(), UG1.cpu().numpy(), int(hits.value)


@pytest.mark.parametrize('speculate', [0, 1])
@pytest.mark.parametrize('name', list(KC.SWEEP_CASES))
def test_direct_sweep_vs_oracle_loop(gpu, name, speculate, monkeypatch):
    """U1 and UG1 bitwise the oracle's loop; with re-speculation off (NNGP_RESPEC_W=0) the hit
    count is the number of slices whose guessed query selects the actual query's list, by the
    oracle; with the default window the re-guessed slices may add hits (printed)."""
    S = KC.sweep_case(name)
    monkeypatch.setenv('NNGP_RESPEC_W', '0')
    U1, UG1, hits = _sweep(gpu, S, speculate)
    assert np.array_equal(U1, S['U1']) and np.array_equal(UG1[1:], S['UG1'][1:])
    assert hits == (sum(S['hit']) if speculate else 0), (hits, S['hit'])
    monkeypatch.delenv('NNGP_RESPEC_W')
    U1w, UG1w, hits_w = _sweep(gpu, S, speculate)
    print(f'{name} speculate={speculate}: hits {hits} without re-speculation (oracle {S["hit"]}), {hits_w} with')
    assert np.array_equal(U1w, S['U1']) and np.array_equal(UG1w[1:], S['UG1'][1:])
    assert hits_w >= 1 if speculate else hits_w == 0
    if speculate:
        _SWEEP_FIRST[name] = (U1w, UG1w)


@pytest.mark.parametrize('knob', ['NNGP_CHAIN=1', 'NNGP_GDIST=0', 'NNGP_HIT_MEAN=0', 'NNGP_KEY_LDS=0',
                                  'NNGP_SPEC_OVERLAP=0'])
@pytest.mark.parametrize('name', list(KC.SWEEP_CASES))
def test_direct_sweep_knobs_are_bitwise_neutral(gpu, name, knob, monkeypatch):
    S = KC.sweep_case(name)
    if name not in _SWEEP_FIRST:
        _SWEEP_FIRST[name] = _sweep(gpu, S, 1)[:2]
    monkeypatch.setenv(*knob.split('='))
    U1, UG1, hits = _sweep(gpu, S, 1)
    assert hits >= 1
    assert np.array_equal(U1, _SWEEP_FIRST[name][0]) and np.array_equal(UG1, _SWEEP_FIRST[name][1])
    assert np.array_equal(U1, S['U1'])
