"""CPU half of the kNN matrix (tests/knn_cases.py): the oracle's select (oracle/nngp_oracle.c
orc_knn) against numpy's stable argsort on every case -- ties, NaN, +inf and subnormal distances
included, which tests/golden/knn.npz does not have -- and the input conditions that make each case
reach the form of the GPU select it is meant for (tests/test_gpu_knn_matrix.py runs them there)."""
import numpy as np
import pytest

import oracle as O
import knn_cases as KC


@pytest.mark.parametrize('case', KC.CASES, ids=KC.CASE_IDS)
def test_oracle_knn_equals_numpy_stable_argsort(case):
    X, q = KC.build(case)
    m = case['m']
    assert X.shape[0] == KC.case_rows(case) and 1 <= m <= min(64, X.shape[0])
    ri, rd, s = KC.ref_knn(X, q, m)
    oi, od = O.knn(X, q, m)
    assert np.array_equal(oi, ri)
    assert np.array_equal(od, rd, equal_nan=True)
    nc = KC.n_candidates(s, m)
    if case['side'] == 'threshold':
        assert nc <= KC.SEL_CAND, nc
    elif case['side'] == 'rounds':
        assert nc > KC.SEL_CAND, nc
    if case['kind'] == 'tie':      # the first m copies by index, all at one distance
        pos = KC.tie_positions(case)
        assert nc == case['L']
        assert np.array_equal(ri, pos[:m]) and len(set(rd.tolist())) == 1
        assert np.sort(s)[case['L']:].min(initial=np.inf) >= 100.0   # every other row >= 10 away
    if case['kind'] == 'low':      # one high word, all distances distinct: ranked on the low word
        assert nc == case['rows'] and len(np.unique(s)) == case['rows']
        assert len(np.unique(s.view(np.uint64) >> np.uint64(32))) == 1


def test_case_table_covers_every_select_form():
    """Each instantiation (by ceil(rows/256)) meets both algorithms, and the candidate count sits
    on both sides of SEL_CAND exactly."""
    form = lambda rows: next((k for k in (2, 4, 8, 16) if rows <= 256 * k), 0)
    sides = set()
    for c in KC.CASES:   # the algorithm a case reaches, from its data (the random cases: the threshold)
        nc = KC.n_candidates(KC.ref_knn(*KC.build(c), c['m'])[2], c['m'])
        sides.add((form(KC.case_rows(c)), 'threshold' if nc <= KC.SEL_CAND else 'rounds'))
    assert sides >={(k, s) for k in (2, 4, 8, 16, 0) for s in ('threshold', 'rounds')}
    L = {c['L'] for c in KC.CASES if c['kind'] == 'tie'}
    assert {256, 257} <= L
    rows = {KC.case_rows(c) for c in KC.CASES}
    assert rows >= {512, 513, 1024, 1025, 2048, 2049, 4096, 4097, KC.KEY_LDS_ROWS, KC.KEY_LDS_ROWS + 1}
    assert max(rows) <= 15000


def test_nonfinite_cases_order():
    """What the non-finite cases are there for: +0 first, the subnormal distances next, and the
    list of the mostly-NaN set running through +inf into the NaN rows in index order."""
    R = KC.NONFINITE_ROWS
    case = next(c for c in KC.CASES if c['id'] == 'nonfinite-r700-m64')
    X, q = KC.build(case)
    idx, dist, s = KC.ref_knn(X, q, 5)
    assert list(idx[:3]) == [R['zero'], R['sub160'], R['sub155']]
    assert dist[0] == 0.0 and 0.0 < dist[1] < dist[2] < np.finfo(float).tiny
    assert np.isinf(s[[R['pinf'], R['ninf'], R['big']]]).all() and np.isnan(s[[R['nan1'], R['nan_all']]]).all()
    last = np.argsort(s, kind='stable')[-5:]
    assert list(last) == sorted([R['pinf'], R['ninf'], R['big']]) + sorted([R['nan1'], R['nan_all']])
    for cid, n_inf in (('nanfill-r100-m30', 1), ('nanfill-r100-m30-qinf', 15)):
        case = next(c for c in KC.CASES if c['id'] == cid)
        X, q = KC.build(case)
        idx, dist, s = KC.ref_knn(X, q, 30)
        n_fin = int(np.isfinite(dist).sum())
        assert n_fin + n_inf == 16 - (cid.endswith('qinf')) and int(np.isposinf(dist).sum()) == n_inf
        nan_part = idx[n_fin + n_inf:]
        assert np.isnan(dist[n_fin + n_inf:]).all() and len(nan_part) >= 14
        assert np.array_equal(nan_part, np.flatnonzero(np.isnan(s))[:len(nan_part)])


@pytest.mark.parametrize('shape', KC.PREDICT_SHAPES, ids=KC.predict_id)
def test_predict_shapes_sit_where_intended(shape):
    m, d, rows = shape[:3]
    assert 1 <= m <= 64 and m <= rows <= 15000
    X, Y, q = KC.predict_data(shape)
    assert np.isfinite(X).all() and np.isfinite(Y).all()
    if len(shape) > 3:   # the duplicated row: more candidates than the threshold select ranks
        assert KC.n_candidates(KC.ref_knn(X, q, m)[2], m) > KC.SEL_CAND


def test_predict_shapes_cover_every_geometry_form():
    S = [s[:2] for s in KC.PREDICT_SHAPES]
    forms = {KC.geometry_form(m, d) for m, d in S} | {KC.geometry_form(m, d, False) for m, d in S}
    assert forms == {'sequential', 'octet', 'wave', 'pairs'}
    assert {d for _, d in S} >= {7, 8, 9, 128, 129}
    assert {m * (d + 1) for m, d in S if d <= 128} >= {KC.XS_DOUBLES}          # staged at the bound
    assert [KC.staged(*s) for s in [(48, 127), (47, 128), (48, 128), (64, 95), (64, 96), (64, 100)]] == \
        [True, True, False, True, False, False]
    assert any(not KC.staged(m, d) and d <= 128 for m, d in S)                # unstaged octet-sized d
    big = [s for s in KC.PREDICT_SHAPES if s[2] > 4096]
    assert all(KC.staged(s[0], s[1]) for s in big if s[1] <= 128)              # keys and rows share LDS
    assert {s[2] <= KC.KEY_LDS_ROWS for s in big} == {True, False}


@pytest.mark.parametrize('name', list(KC.SWEEP_CASES))
def test_sweep_case_conditions(name):
    """The oracle side of the direct sweep cases: finite iterates, the guess chain hitting beyond
    slice 0 and missing somewhere, and -- with the duplicated row -- selects past SEL_CAND
    candidates for an actual query and for a guess."""
    S = KC.sweep_case(name)
    assert np.isfinite(S['U1']).all() and np.isfinite(S['UG1']).all()
    assert S['hit'][0] and any(S['hit'][1:]) and not all(S['hit'])
    if KC.SWEEP_CASES[name][1]:
        assert max(S['ncand_q']) > KC.SEL_CAND and max(S['ncand_g']) > KC.SEL_CAND
    else:   # the corrected chain follows the fine trajectory; the streaming select
        assert np.max(np.abs(S['U1'] - S['traj'])) < 1e-6 and S['rows'] > 4096
