"""CPU: nngp_predict_batch's boundary without a GPU -- the export, its argument checks (each
reported by name before any HIP call), the empty batch, and the host's chunk rule restated against
the constant include/nngp.h defines."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_Y_MAX = 65535   # blockIdx.y = query within a chunk


def max_fits():
    src = open(os.path.join(ROOT, 'include', 'nngp.h')).read()
    found = re.findall(r'^#define\s+NNGP_PREDICT_BATCH_MAX_FITS\s+(\d+)', src, re.M)
    assert len(found) == 1
    return int(found[0])


def chunk_queries(n_fits, bound=None):
    """Queries per chunk (include/nngp.h): min(65535, max(1, NNGP_PREDICT_BATCH_MAX_FITS / n_fits))."""
    bound = max_fits() if bound is None else bound
    return min(GRID_Y_MAX, max(1, bound // n_fits))


def test_symbol_is_exported_and_bound():
    import nngp_amd
    assert 'nngp_predict_batch' in nngp_amd._lib.EXPORTS
    f = nngp_amd.lib().nngp_predict_batch
    assert f.restype is ctypes.c_int32 and len(f.argtypes) == 20
    assert hasattr(nngp_amd.NNGP_p, 'predict_batch') and hasattr(nngp_amd.NNGP_p, 'predict_batch_device')


def test_argument_errors_are_reported_before_any_hip_call():
    import nngp_amd
    L = nngp_amd.lib()
    jit = (ctypes.c_double * 9)(*range(-20, -11))
    P = 4096   # a non-null address nothing reads: every check comes before the first HIP call
    ok = dict(X=P, Y=P, rows=10, d=3, Q=P, n_q=2, m=5, n_jitter=9, jexp=jit, R=1, theta0=P, maxfev=400, preds=P,
              bias=None, out=None, idx=None, fits=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.nngp_predict_batch(a['X'], a['Y'], a['rows'], a['d'], a['Q'], a['n_q'], a['m'], a['n_jitter'],
                                    a['jexp'], a['R'], a['theta0'], 0.1, 0.1, a['maxfev'], a['preds'], a['bias'],
                                    a['out'], a['idx'], a['fits'], None)

    for kw, text in ((dict(X=None), b'X is NULL'), (dict(Y=None), b'Y is NULL'), (dict(Q=None), b'Q is NULL'),
                     (dict(jexp=None), b'jitter_exp_host is NULL'), (dict(theta0=None), b'theta0 is NULL'),
                     (dict(preds=None), b'preds_out is NULL'), (dict(n_q=-1), b'n_q'), (dict(m=0), b'm='),
                     (dict(m=65, rows=100), b'm='), (dict(m=11), b'm='), (dict(m=5, rows=4), b'rows='),
                     (dict(d=0), b'd must'), (dict(n_jitter=0), b'n_jitter'), (dict(n_jitter=17), b'n_jitter'),
                     (dict(R=0), b'n_restarts'), (dict(maxfev=0), b'maxfev'), (dict(bias=P), b'bias and out'),
                     (dict(out=P), b'bias and out')):
        assert call(**kw) == -1, kw
        assert text in L.nngp_last_error(), (kw, L.nngp_last_error())
        if 'n_q' not in kw:
            assert call(n_q=0, **kw) == -1, kw    # an empty batch is checked too
    assert call(n_q=0) == 0                       # an empty batch is a no-op
    assert call(n_q=0, bias=P, out=P) == 0        # out may be bias itself
    assert call(n_q=0, m=10, idx=P, fits=P) == 0  # m = rows


def test_chunk_rule_against_the_header_constant():
    bound = max_fits()
    assert bound == 262144                                    # the sweep's speculation bound
    assert chunk_queries(27) == bound // 27 == 9709           # d = 3
    assert chunk_queries(288 * 9) == 101                      # FHN-PDE nx = 12: 2 592 fits per query
    assert chunk_queries(800 * 9) == 36
    assert chunk_queries(bound) == 1 and chunk_queries(bound + 1) == 1 and chunk_queries(10 * bound) == 1
    assert chunk_queries(9) == bound // 9 and chunk_queries(4) == GRID_Y_MAX and chunk_queries(1) == GRID_Y_MAX
    for n_fits in (1, 4, 5, 9, 27, 2592, 7200, bound // 2, bound // 2 + 1, bound):
        c = chunk_queries(n_fits)
        assert 1 <= c <= GRID_Y_MAX and (c * n_fits <= bound or c == 1)
        assert c == GRID_Y_MAX or (c + 1) * n_fits > bound    # the largest chunk the two bounds allow
