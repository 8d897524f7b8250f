"""Correction models -- the reference's ModelAbstr / BareParareal / NNGP_p plugin surface
(models.py:19-270) with the nearest-neighbour GP running on the GPU.

NNGP_p keeps the reference's constructor arguments (n, N, worker_pool, theta, fatol, xatol, nn,
seed, n_restarts, ...), its RNG (np.random.default_rng(seed), models.py:114) and the exact order
of its draws: per prediction, rng.integers(-8, 0, 2) once for every (coordinate, jitter,
restart) in itertools.product order (models.py:186-192).  A single vectorised
rng.integers(-8, 0, (count, 2)) yields the same stream (the range is a power of two, so
numpy's Lemire sampler never rejects; pinned by tests/test_host.py against tests/golden/rng.npz).

Compute paths (all HIP, no CPU fallback):
  predict(...)         reference signature, host arrays in/out -> nngp_predict (fused kernels)
  predict_device(...)  device tensors, used by the Parareal driver's sequential loop
  predict_batch(...) / predict_batch_device(...)  many independent queries -> nngp_predict_batch,
                       each bitwise its predict (the driver's model comparison)
  get_preds(...)       reference signature on pre-selected (xm, ym) -> nngp_nm_fit_batch +
                       first-argmin + nngp_gp_mean (the unfused path of the same kernels)

GPjax_p (models.py:273-473) is the full-data GParareal model: per coordinate and jitter a
Nelder-Mead fit of the GP over ALL training rows, warm-started at the previous optimum, batched
across fits on the GPU (nngp_gpfull_fit), and posterior means from the memoised Cholesky weights
(nngp_gpfull_mean / the native sweep).
"""
import copy
import ctypes
import time
from itertools import product

import numpy as np

from . import _lib

JITTERS = np.arange(-20, -11, dtype=float)   # models.py:186
MAX_NEIGHBOURS = 64   # the HIP fits' largest padded kernel size (include/nngp.h)


class ModelAbstr():

    def __init__(self, **kwargs):
        self.train_time = 0
        self.pred_time = 0
        N = kwargs['N']
        self.pred_times = np.zeros(N)
        self.time_k = 0

    def fit_timed(self, x, y, *args, **kwargs):
        self.time_k = kwargs['k']
        s_time = time.time()
        ret = self.fit(x, y, *args, **kwargs)
        elap_time = time.time() - s_time
        self.train_time += elap_time
        self.pred_times[self.time_k] += elap_time
        return ret

    def predict_timed(self, new_x, *args, **kwargs):
        s_time = time.time()
        ret = self.predict(new_x, *args, **kwargs)
        elap_time = time.time() - s_time
        self.pred_time += elap_time
        self.pred_times[self.time_k] += elap_time
        return ret

    def add_pred_time(self, seconds):
        """Device-measured prediction time (the Parareal driver times whole sweeps with events)."""
        self.pred_time += seconds
        self.pred_times[self.time_k] += seconds

    def get_times(self):
        return {'mdl_train_t': self.train_time, 'mdl_pred_t': self.pred_time,
                'mdl_tot_t': self.train_time + self.pred_time, 'by_iter': self.pred_times[:self.time_k + 1]}

    def fit(self, x, y, *args, **kwargs):
        self.x, self.y = x, y
        raise Exception('Not implemented')

    def predict(self, new_x, prev_F, prev_G):
        raise Exception('Not implemented')

    def state_dict(self):
        """Counters for a store_int checkpoint (JSON-serialisable)."""
        return {'name': self.name, 'train_time': self.train_time, 'pred_time': self.pred_time,
                'pred_times': self.pred_times.tolist(), 'time_k': self.time_k, 'settings': {}}

    def load_state(self, st):
        self.train_time, self.pred_time = st['train_time'], st['pred_time']
        self.pred_times = np.array(st['pred_times'], dtype=float)
        self.time_k = st['time_k']

    def store(self):
        if hasattr(self, 'pool'):
            pool = self.pool
            self.pool = None
            new = copy.deepcopy(self)
            self.pool = pool
        else:
            new = copy.deepcopy(self)
        return new


class BareParareal(ModelAbstr):
    """Classic Parareal correction F - G (models.py:74-83)."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.name = 'Parareal'

    def fit(self, *args, **kwargs):
        pass

    def predict(self, new_x, prev_F, prev_G, *args, **kwargs):
        return prev_F - prev_G


class NNGP_p(ModelAbstr):
    """Nearest-neighbour GP correction (models.py:98-270) on the GPU."""

    def __init__(self, n, N, worker_pool=None, theta=None, fatol=None, xatol=None, **kwargs):
        super().__init__(N=N, **kwargs)
        if theta is None:
            theta = [1, 1]
        self.theta = np.array(theta)
        self.name = 'NNGP'
        self.fatol = 1e-1 if fatol is None else fatol
        self.xatol = 1e-1 if xatol is None else xatol
        self.n = n
        self.n_restarts = kwargs.get('n_restarts', 1)
        self.nn = kwargs.get('nn', 'adaptive')
        self.seed = kwargs.get('seed', 45)
        self.rng = np.random.default_rng(self.seed)
        np.random.seed(self.seed)
        self.pool = worker_pool
        self.maxfev = 200 * len(self.theta)   # scipy default maxiter = maxfev = 200*N
        self.tot_train_t = 0
        self.train_count = 0
        self.k = 0
        self._dev_xy = None
        self._host_xy = None
        if self.nn != 'adaptive' and not 1 <= int(self.nn) <= MAX_NEIGHBOURS:
            raise ValueError(f'nn={self.nn}: the GPU nnGP correction supports 1..{MAX_NEIGHBOURS} neighbours')

    # ------------------------------------------------------------------------------ helpers
    @property
    def n_fits(self):
        return self.n * len(JITTERS) * self.n_restarts

    def n_neighbours(self):
        m = max(10, self.k + 2) if self.nn == 'adaptive' else int(self.nn)   # models.py:172-175
        if m > MAX_NEIGHBOURS:   # adaptive m = k+2 passes the bound at iteration k = 63
            raise ValueError(f"nn='adaptive' asks for m={m} neighbours at iteration {self.k}; the GPU nnGP "
                             f'correction supports up to {MAX_NEIGHBOURS}')
        return m

    def draw_thetas(self, n_predictions):
        """Initial thetas for `n_predictions` consecutive predictions (models.py:192)."""
        return self.rng.integers(-8, 0, (n_predictions * self.n_fits, len(self.theta))).astype(np.float64)

    def get_times(self):
        out = super().get_times()
        out.update({'serial_train_time': self.tot_train_t, 'calc_detail_avg': None, 'overhead': None,
                    'avg_serial_train_time': self.tot_train_t / max(self.train_count, 1)})
        return out

    def fit(self, x, y, k, *args, **kwargs):
        """models.py:157-159.  The Parareal driver hands over its device-resident training set
        (torch tensors): those are kept for the device path, and `x` / `y` stay host arrays as in
        the reference (copied from the device on first access)."""
        self.k = k
        if hasattr(x, 'data_ptr'):
            self._dev_xy = (x, y)
            self._host_xy = None
        else:
            self._dev_xy = None
            self._host_xy = (x, y)

    def _host(self):
        if self._host_xy is None:
            if self._dev_xy is None:
                raise AttributeError("'NNGP_p' has no training set yet: call fit(x, y, k) first")
            self._host_xy = tuple(v.detach().cpu().numpy() for v in self._dev_xy)
        return self._host_xy

    def _set_xy(self, i, v):
        """Reference-style assignment `mdl.x = ...` / `mdl.y = ...` (plain attributes there,
        models.py:157-159): the host pair is updated and the device copy dropped, so the next
        prediction uploads the assigned set."""
        pair = list(self._host_xy) if self._host_xy is not None else (
            [v_.detach().cpu().numpy() for v_ in self._dev_xy] if self._dev_xy is not None else [None, None])
        pair[i] = v
        self._host_xy = tuple(pair)
        self._dev_xy = None

    x = property(lambda self: self._host()[0], lambda self, v: self._set_xy(0, v))
    y = property(lambda self: self._host()[1], lambda self, v: self._set_xy(1, v))

    # ---------------------------------------------------------------------------- device path
    def predict_device(self, X, Y, rows, new_x, theta0, out=None, bias=None, preds=None,
                       fits_out=None, stream=None):
        """One correction on device tensors.  X/Y: [>=rows][n] training set, new_x: [n],
        theta0: [n_fits][2] (this prediction's draws).  Writes preds (and out = preds + bias)."""
        import torch
        m = min(self.n_neighbours(), int(rows))   # argsort(...)[:nn] on fewer rows keeps them all
        if preds is None:
            preds = torch.empty(self.n, dtype=torch.float64, device=X.device)
        jit, jp = _lib.host_doubles(JITTERS)
        st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().nngp_predict(
            X.data_ptr(), Y.data_ptr(), int(rows), self.n, new_x.data_ptr(), m, len(jit), jp,
            self.n_restarts, theta0.data_ptr(), float(self.fatol), float(self.xatol), self.maxfev,
            preds.data_ptr(), bias.data_ptr() if bias is not None else None,
            out.data_ptr() if out is not None else None,
            fits_out.data_ptr() if fits_out is not None else None, st))
        self.train_count += self.n_fits
        return preds

    def device_xy(self):
        """(X, Y) on the device, uploading a host training set given to fit() (or assigned)."""
        if self._dev_xy is None:
            if self._host_xy is None or self._host_xy[0] is None or self._host_xy[1] is None:
                raise AttributeError("'NNGP_p' has no training set yet: call fit(x, y, k) first")
            self._dev_xy = (_lib.as_device(self._host_xy[0]), _lib.as_device(self._host_xy[1]))
        return self._dev_xy

    def predict_batch_device(self, Q, theta0=None, out=None, bias=None, preds=None, idx_out=None, fits_out=None,
                             stream=None):
        """Independent corrections at every row of Q [nq][n] on the model's device training set, one
        launch set (nngp_predict_batch): row q is predict_device(X, Y, rows, Q[q], theta0[q]) bit
        for bit.  theta0: [nq][n_fits][2] (or [nq * n_fits][2]); None draws it here -- the RNG stream
        of nq consecutive predict calls.  Writes preds [nq][n] (and out = preds + bias, given
        together; out may be bias itself), optionally idx_out int32 [nq][m] (the ordered neighbour
        lists) and fits_out [nq][n_fits][4]."""
        import torch
        X, Y = self.device_xy()
        rows, n = int(X.shape[0]), self.n
        if X.dim() != 2 or int(X.shape[1]) != n or rows < 1:
            raise ValueError(f'the training set must be [rows >= 1][{n}] (got x of shape {tuple(X.shape)})')
        _knn_tensor(X, 'x', X.shape, X.device)
        _knn_tensor(Y, 'y', X.shape, X.device)
        m = min(self.n_neighbours(), rows)   # argsort(...)[:nn] on fewer rows keeps them all
        if not torch.is_tensor(Q) or Q.dim() != 2:
            raise ValueError('Q must be a device tensor of shape [n_q][n]')
        nq, nf = int(Q.shape[0]), self.n_fits
        q_ptr = _knn_tensor(Q, 'Q', (nq, n), X.device)
        if (out is None) != (bias is None):
            raise ValueError('out and bias go together')
        if theta0 is None:
            theta0 = torch.tensor(self.draw_thetas(nq), dtype=torch.float64, device=X.device)
        flat = torch.is_tensor(theta0) and tuple(theta0.shape) == (nq * nf, 2)
        th_ptr = _knn_tensor(theta0, 'theta0', (nq * nf, 2) if flat else (nq, nf, 2), X.device)
        if preds is None:
            preds = torch.empty((nq, n), dtype=torch.float64, device=X.device)
        if nq == 0:   # (an empty tensor has no address to hand over)
            return preds
        ptr = lambda t, name, shape, dtype=None: None if t is None else _knn_tensor(t, name, shape, X.device, dtype)
        jit, jp = _lib.host_doubles(JITTERS)
        st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().nngp_predict_batch(
            X.data_ptr(), Y.data_ptr(), rows, n, q_ptr, nq, m, len(jit), jp, self.n_restarts, th_ptr,
            float(self.fatol), float(self.xatol), self.maxfev, ptr(preds, 'preds', (nq, n)),
            ptr(bias, 'bias', (nq, n)), ptr(out, 'out', (nq, n)), ptr(idx_out, 'idx_out', (nq, m), torch.int32),
            ptr(fits_out, 'fits_out', (nq, nf, 4)), st))
        self.train_count += nq * nf
        return preds

    # ------------------------------------------------------------------------- reference API
    def predict_batch(self, new_x):
        """predict at every row of new_x [nq][n] (host arrays in/out): what nq consecutive predict
        calls return, RNG stream included, as one launch set."""
        torch = _lib.require_gpu()
        Q = torch.tensor(np.ascontiguousarray(np.asarray(new_x, dtype=np.float64).reshape(-1, self.n)), device='cuda')
        return self.predict_batch_device(Q).cpu().numpy()

    def predict(self, new_x, prev_F=None, prev_G=None, *args, **kwargs):
        """models.py:171-183 (host arrays in/out; kNN + fits + argmin + mean on the GPU)."""
        torch = _lib.require_gpu()
        X, Y = self.device_xy()
        q = torch.tensor(np.asarray(new_x, dtype=np.float64).reshape(-1), device='cuda')
        th0 = torch.tensor(self.draw_thetas(1), device='cuda')
        preds = self.predict_device(X, Y, X.shape[0], q, th0)
        return preds.cpu().numpy()

    def get_preds(self, xm, ym, n, new_x, intrvl_i):
        """models.py:185-226 on already-selected neighbours: all fits, first argmin, mean."""
        torch = _lib.require_gpu()
        m = xm.shape[0]
        ins = list(product(range(n), range(len(JITTERS)), range(self.n_restarts)))
        th0 = self.draw_thetas(1)
        res = self.fit_batch(xm, ym, [i[0] for i in ins], [i[1] for i in ins], th0)
        preds = np.empty(n)
        best_th = np.empty((n, 2))
        best_j = np.empty(n, dtype=np.int32)
        per = len(JITTERS) * self.n_restarts
        for j in range(n):
            fv = res['fval'][j * per:(j + 1) * per]
            b = int(np.argmin(fv))                  # first minimum == models.py:212-215
            best_th[j] = res['theta'][j * per + b]
            best_j[j] = ins[j * per + b][1]
        preds[:] = self.gp_mean(xm, ym, new_x, best_th, best_j)
        return preds

    def fit_batch(self, xm, ym, coords, jitter_idx, theta0):
        """pool.map(_get_opt_par, ...) as one launch (nngp_nm_fit_batch)."""
        torch = _lib.require_gpu()
        xm_t = torch.tensor(np.ascontiguousarray(xm, dtype=np.float64), device='cuda')
        ym_t = torch.tensor(np.ascontiguousarray(ym, dtype=np.float64), device='cuda')
        nf = len(coords)
        c_t = torch.tensor(np.asarray(coords, dtype=np.int32), device='cuda')
        j_t = torch.tensor(np.asarray(jitter_idx, dtype=np.int32), device='cuda')
        th_t = torch.tensor(np.ascontiguousarray(theta0, dtype=np.float64), device='cuda')
        th_o = torch.empty((nf, 2), dtype=torch.float64, device='cuda')
        fv_o = torch.empty(nf, dtype=torch.float64, device='cuda')
        ne_o = torch.empty(nf, dtype=torch.int32, device='cuda')
        jit, jp = _lib.host_doubles(JITTERS)
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().nngp_nm_fit_batch(
            xm.shape[0], xm.shape[1], xm_t.data_ptr(), ym_t.data_ptr(), nf, c_t.data_ptr(), j_t.data_ptr(),
            len(jit), jp, th_t.data_ptr(), float(self.fatol), float(self.xatol), self.maxfev,
            th_o.data_ptr(), fv_o.data_ptr(), ne_o.data_ptr(), st))
        self.train_count += nf
        return {'theta': th_o.cpu().numpy(), 'fval': fv_o.cpu().numpy(), 'nfev': ne_o.cpu().numpy()}

    def gp_mean(self, xm, ym, new_x, theta, jitter_idx):
        torch = _lib.require_gpu()
        n = ym.shape[1]
        xm_t = torch.tensor(np.ascontiguousarray(xm, dtype=np.float64), device='cuda')
        ym_t = torch.tensor(np.ascontiguousarray(ym, dtype=np.float64), device='cuda')
        q = torch.tensor(np.asarray(new_x, dtype=np.float64).reshape(-1), device='cuda')
        th = torch.tensor(np.ascontiguousarray(theta, dtype=np.float64), device='cuda')
        ji = torch.tensor(np.asarray(jitter_idx, dtype=np.int32), device='cuda')
        out = torch.empty(n, dtype=torch.float64, device='cuda')
        jit, jp = _lib.host_doubles(JITTERS)
        _lib.check(_lib.lib().nngp_gp_mean(xm.shape[0], n, xm_t.data_ptr(), ym_t.data_ptr(), q.data_ptr(),
                                            th.data_ptr(), ji.data_ptr(), len(jit), jp, out.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream))
        return out.cpu().numpy()

    @staticmethod
    def _get_opt_par(static_ins, ins, rnd):
        """models.py:228-237: one fit -> (*theta, fval, jitter, j, elapsed)."""
        st_ = time.time()
        xm, ym, fatol, xatol = static_ins
        j, jitter, _ = ins
        tmp = NNGP_p(n=ym.shape[1], N=1, fatol=fatol, xatol=xatol)
        jidx = int(np.where(JITTERS == jitter)[0][0])
        r = tmp.fit_batch(xm, ym, [j], [jidx], np.asarray(rnd, dtype=float).reshape(1, 2))
        return (*r['theta'][0], r['fval'][0], jitter, j, time.time() - st_)

    def store(self):
        """A deep copy for the result dict (models.py store): host x / y, no device tensors."""
        if self._dev_xy is not None:
            self._host()
        dev, self._dev_xy = self._dev_xy, None
        try:
            new = super().store()
        finally:
            self._dev_xy = dev
        new.pool = None
        return new

    def state_dict(self):
        st = super().state_dict()
        st['settings'] = {'theta': self.theta.tolist(), 'fatol': self.fatol, 'xatol': self.xatol,
                          'n_restarts': self.n_restarts, 'nn': self.nn, 'seed': self.seed}
        st.update({'k': self.k, 'tot_train_t': self.tot_train_t, 'train_count': self.train_count,
                   'rng': self.rng.bit_generator.state})
        return st

    def load_state(self, st):
        super().load_state(st)
        self.k, self.tot_train_t, self.train_count = st['k'], st['tot_train_t'], st['train_count']
        self.rng.bit_generator.state = st['rng']

    def restore_attrs(self, pool):
        self.pool = pool


NNTYPES = ('nn', 'col+rnd', 'col_only', 'row_col', 'row', 'col_full')
ALTERNATION_TURNS = 101   # the reference's cycler leaves its loop after turn c == 100 (nnGPara_with_time.py:112)


def _alternation(i, N):
    """The intervals i, i+1, i-1, i+2, ... as the reference's my_cycler yields them
    (nnGPara_with_time.py:98-115): a turn takes the next interval downwards, then the next upwards; a
    side that has run out is skipped, the loop ends in the turn that finds both run out, and after
    ALTERNATION_TURNS turns whatever is left."""
    lo, hi = i, i + 1
    for _ in range(ALTERNATION_TURNS):
        lo_out = lo < 0
        if not lo_out:
            yield lo
            lo -= 1
        if hi < N:
            yield hi
            hi += 1
        elif lo_out:
            return


class NNGP_alt(NNGP_p):
    """The reference's neighbour-set variants of nnGParareal (NNGP_alt, nnGPara_with_time.py:27-184):
    the nnGP correction on neighbours chosen by their place in the (interval, iteration) table of
    starting values instead of by distance.  nntype 'nn' is NNGP_p itself.  For the others the list
    of slice i at iteration k depends on (i, k), the table's NaN pattern and (col+rnd) the model's
    second generator only -- never on the query -- so neighbour_lists gives every slice's list
    before the sweep, and the device runs them as prescribed lists (nngp_listed_sweep /
    nngp_predict_listed).  Cells are written (interval, iteration):
      col_only  (i, 0) .. (i, k): m = k + 1, nn is not used
      col+rnd   c = min(nn, k+1) cells (i, k+1-c) .. (i, k), then of the first nn entries of
                rng2.permutation(rows) (one draw per slice, in slice order) those that are not the
                first training row sharing a coordinate value with one of the column rows, nn - c of them
      row_col   every filled cell by |k' - k| + |i' - i|, ties interval-major (the reference's tie order
                is numpy's unstable argsort's: DESIGN.md 3.3c)
      row       iterations k, k-1, .., 0; in each the intervals i, i+1, i-1, i+2, ..
      col_full  intervals i, i+1, i-1, ..; in each the iterations k, .., 0
    with empty (NaN) cells skipped, at most 101 alternation turns, and the first nn taken.  nn follows
    n_neighbours() (the reference reads self.nn directly for the last three, so 'adaptive' fails there)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        nntype = kwargs.get('nntype')
        if nntype not in NNTYPES:
            raise ValueError(f'nntype={nntype!r}: expected one of {NNTYPES}')
        self.nntype = nntype
        self.name = 'NNGP' + str(nntype)
        self.rng2 = np.random.default_rng(self.seed)
        self.data_x = None
        self._cells = None

    @property
    def listed(self):
        """The neighbours are prescribed lists (every nntype but 'nn')."""
        return self.nntype != 'nn'

    def fit(self, x, y, k, *args, **kwargs):
        """The parent's fit, plus the table data_x [N][n][>= k+1] (kept, not copied: NaN where an
        interval had converged) and the cell -> training-row map.  The driver appends the filled
        intervals of column k' as one block per iteration, so
            row(i, k') = off[k'] + i - first[k'],   first[k'] = the first filled interval of column k'."""
        super().fit(x, y, k, *args, **kwargs)
        if not self.listed:
            return
        data_x = kwargs.get('data_x')
        if data_x is None:
            raise NotImplementedError(f"nntype='{self.nntype}' selects neighbours from the table of starting "
                                      "values: fit needs data_x (PararealLight and the lag_k training sets keep none)")
        filled = ~np.isnan(data_x[:, :, :k + 1]).any(axis=1)   # [N][k+1]
        N = filled.shape[0]
        count = filled.sum(axis=0)
        first = np.where(count > 0, filled.argmax(axis=0), N)
        if not all(filled[first[c]:, c].all() for c in range(k + 1)):
            raise ValueError('data_x: the filled intervals of a column must be one block up to the last interval')
        off = np.concatenate([[0], np.cumsum(count)])
        if off[-1] != int(np.shape(x)[0]):
            raise ValueError(f'data_x holds {off[-1]} filled cells up to iteration {k} but the training set has '
                             f'{int(np.shape(x)[0])} rows')
        self.data_x = data_x
        self._cells = (filled, first, off[:-1])

    def cell_row(self, i, kk):
        """The training row of cell (interval i, iteration kk)."""
        filled, first, off = self._cells
        if not filled[i, kk]:
            raise ValueError(f'cell (interval {i}, iteration {kk}) is empty')
        return int(off[kk] + i - first[kk])

    def _host_x(self):
        """The training inputs on the host, from the table (no device copy): block k' = column k'."""
        filled, first, _ = self._cells
        return np.concatenate([self.data_x[first[c]:, :, c] for c in range(filled.shape[1])])

    def list_size(self):
        """m of this iteration's lists."""
        if self.nntype == 'col_only':
            m = self.k + 1
            if m > MAX_NEIGHBOURS:
                raise ValueError(f"nntype='col_only' asks for m={m} neighbours at iteration {self.k}; the GPU nnGP "
                                 f'correction supports up to {MAX_NEIGHBOURS}')
            return m
        return self.n_neighbours()

    def _cells_of(self, i, nn):
        """The first nn filled cells (interval, iteration) of slice i in the order of self.nntype."""
        filled, k = self._cells[0], self.k
        N = filled.shape[0]
        if self.nntype == 'row_col':
            dist = np.abs(np.arange(k + 1)[None, :] - k) + np.abs(np.arange(N)[:, None] - i)
            flat = np.argsort(dist, axis=None, kind='stable')
            flat = flat[filled.reshape(-1)[flat]][:nn]
            return [(int(f // (k + 1)), int(f % (k + 1))) for f in flat]
        if self.nntype == 'row':
            order = ((c, kk) for kk in range(k, -1, -1) for c in _alternation(i, N))
        else:   # col_full
            order = ((c, kk) for c in _alternation(i, N) for kk in range(k, -1, -1))
        cells = []
        for c, kk in order:
            if filled[c, kk]:
                cells.append((c, kk))
                if len(cells) == nn:
                    break
        return cells

    def neighbour_lists(self, I, N):
        """int32 [N-I][m]: the ordered training rows of slices i = I .. N-1 at the fitted iteration
        (consumes one rng2 permutation per slice for col+rnd).  ValueError where a slice has fewer than
        m candidates (the reference dies there on an exhausted generator)."""
        if not self.listed:
            raise ValueError("nntype='nn' has no prescribed lists: its neighbours depend on the query")
        if self._cells is None:
            raise AttributeError("'NNGP_alt' has no table yet: call fit(x, y, k, data_x=...) first")
        k, m = self.k, self.list_size()
        rows = int(self._cells[2][-1] + self._cells[0][:, -1].sum())
        out = np.empty((max(N - I, 0), m), dtype=np.int32)
        x = self._host_x() if self.nntype == 'col+rnd' else None
        for i in range(I, N):
            if self.nntype == 'col_only':
                lst = [self.cell_row(i, kk) for kk in range(k + 1)]
            elif self.nntype == 'col+rnd':
                c = min(m, k + 1)
                lst = [self.cell_row(i, kk) for kk in range(k + 1 - c, k + 1)]
                # the first training row with ANY coordinate equal to the column row (np.any(x == row,
                # axis=1).argmax(), nnGPara_with_time.py:62) -- not necessarily the row itself
                removed = {int(np.argmax(np.any(x == x[r][None, :], axis=1))) for r in lst}
                cands = self.rng2.permutation(rows)[:m]
                lst += [int(r) for r in cands if int(r) not in removed][:m - c]
            else:
                lst = [self.cell_row(c, kk) for c, kk in self._cells_of(i, m)]
            if len(lst) < m:
                raise ValueError(f"nntype='{self.nntype}' at iteration {k}, interval {i}: {len(lst)} neighbours "
                                 f'are available, {m} are needed')
            out[i - I] = lst
        return out

    # ---------------------------------------------------------------------------- device path
    def predict_listed_device(self, Q, lists, theta0=None, out=None, bias=None, preds=None, fits_out=None,
                              stream=None):
        """Corrections at every row of Q [nq][n] on the prescribed lists [nq][m] (host int32), one launch
        set (nngp_predict_listed).  Arguments as predict_batch_device."""
        import torch
        X, Y = self.device_xy()
        rows, n = int(X.shape[0]), self.n
        _knn_tensor(X, 'x', (rows, n), X.device)
        _knn_tensor(Y, 'y', (rows, n), X.device)
        if not torch.is_tensor(Q) or Q.dim() != 2:
            raise ValueError('Q must be a device tensor of shape [n_q][n]')
        nq, nf = int(Q.shape[0]), self.n_fits
        lists = np.ascontiguousarray(lists, dtype=np.int32)
        if lists.ndim != 2 or lists.shape[0] != nq:
            raise ValueError(f'lists must be [{nq}][m] (got {lists.shape})')
        m = int(lists.shape[1])
        q_ptr = _knn_tensor(Q, 'Q', (nq, n), X.device)
        if (out is None) != (bias is None):
            raise ValueError('out and bias go together')
        if theta0 is None:
            theta0 = torch.tensor(self.draw_thetas(nq), dtype=torch.float64, device=X.device)
        flat = torch.is_tensor(theta0) and tuple(theta0.shape) == (nq * nf, 2)
        th_ptr = _knn_tensor(theta0, 'theta0', (nq * nf, 2) if flat else (nq, nf, 2), X.device)
        if preds is None:
            preds = torch.empty((nq, n), dtype=torch.float64, device=X.device)
        if nq == 0:
            return preds
        ptr = lambda t, name, shape: None if t is None else _knn_tensor(t, name, shape, X.device)
        jit, jp = _lib.host_doubles(JITTERS)
        st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().nngp_predict_listed(
            X.data_ptr(), Y.data_ptr(), rows, n, q_ptr, nq, lists.ctypes.data, m, len(jit), jp, self.n_restarts,
            th_ptr, float(self.fatol), float(self.xatol), self.maxfev, ptr(preds, 'preds', (nq, n)),
            ptr(bias, 'bias', (nq, n)), ptr(out, 'out', (nq, n)), ptr(fits_out, 'fits_out', (nq, nf, 4)), st))
        self.train_count += nq * nf
        return preds

    def predict_device(self, X, Y, rows, new_x, theta0, out=None, bias=None, preds=None, fits_out=None, stream=None,
                       i=None):
        """One correction on device tensors; for a listed nntype the neighbours are interval i's
        (one nngp_predict_listed query on the model's training set, which is the driver's X / Y)."""
        if not self.listed:
            return super().predict_device(X, Y, rows, new_x, theta0, out=out, bias=bias, preds=preds,
                                          fits_out=fits_out, stream=stream)
        if i is None:
            raise ValueError(f"nntype='{self.nntype}' predicts for an interval: pass i")
        one = lambda t: None if t is None else t.reshape(1, -1)
        if preds is None:
            import torch
            preds = torch.empty(self.n, dtype=torch.float64, device=new_x.device)
        self.predict_listed_device(one(new_x), self.neighbour_lists(i, i + 1), theta0=theta0.reshape(1, -1, 2),
                                   out=one(out), bias=one(bias), preds=one(preds),
                                   fits_out=None if fits_out is None else fits_out.reshape(1, -1, 4), stream=stream)
        return preds

    def predict_batch_device(self, Q, theta0=None, out=None, bias=None, preds=None, idx_out=None, fits_out=None,
                             stream=None, intervals=None):
        """predict_batch_device; for a listed nntype Q[j] is the starting value of interval intervals[j]
        (consecutive: the driver's slices) and idx_out receives no list (they are neighbour_lists')."""
        if not self.listed:
            return super().predict_batch_device(Q, theta0=theta0, out=out, bias=bias, preds=preds, idx_out=idx_out,
                                                fits_out=fits_out, stream=stream)
        if intervals is None or idx_out is not None:
            raise ValueError(f"nntype='{self.nntype}': pass the queries' intervals=(I, N) and no idx_out")
        I, N = intervals
        return self.predict_listed_device(Q, self.neighbour_lists(I, N), theta0=theta0, out=out, bias=bias,
                                          preds=preds, fits_out=fits_out, stream=stream)

    def predict(self, new_x, prev_F=None, prev_G=None, *args, **kwargs):
        """The reference's predict (host arrays in / out); a listed nntype needs the interval, i=."""
        if not self.listed:
            return super().predict(new_x, prev_F, prev_G, *args, **kwargs)
        torch = _lib.require_gpu()
        if kwargs.get('i') is None:
            raise ValueError(f"nntype='{self.nntype}' predicts for an interval: pass i=")
        X, Y = self.device_xy()
        q = torch.tensor(np.asarray(new_x, dtype=np.float64).reshape(-1), device='cuda')
        th0 = torch.tensor(self.draw_thetas(1), device='cuda')
        return self.predict_device(X, Y, X.shape[0], q, th0, i=int(kwargs['i'])).cpu().numpy()

    def store(self):
        table, self.data_x = self.data_x, None   # the driver's own array: the result dict has it already
        try:
            new = super().store()
        finally:
            self.data_x = table
        return new

    def state_dict(self):
        st = super().state_dict()
        st['settings']['nntype'] = self.nntype
        st['rng2'] = self.rng2.bit_generator.state
        return st

    def load_state(self, st):
        super().load_state(st)
        if 'rng2' in st:
            self.rng2.bit_generator.state = st['rng2']


def _select_fit(theta, fval, jitter):
    """The per-coordinate choice of models.py:388-395 / 361-365: keep fits with
    fval < 0.9 * min(fval) (all if none), then the first minimum in order (Python min, '<')."""
    fmin = np.min(fval)
    mask = fval < fmin * 0.9
    if mask.sum() == 0:
        mask[:] = True
    idx = np.nonzero(mask)[0]
    best = idx[0]
    for i in idx[1:]:
        if fval[i] < fval[best]:
            best = i
    return tuple(float(v) for v in theta[best]), float(fval[best]), float(jitter[best])


def _group_world(group):
    """(world, rank) of a torch.distributed group, (1, 0) without one."""
    import torch.distributed as dist
    if group is False or not (dist.is_available() and dist.is_initialized()):
        return 1, 0
    return dist.get_world_size(group), dist.get_rank(group)


def _gather_rows(local, group, world):
    """All-gather of equal [chunk][...] fp64 blocks in rank order over `group`: RCCL's
    all_gather_into_tensor on device tensors (an NCCL group), gloo's list form through host memory
    (several ranks sharing one GPU)."""
    import torch
    import torch.distributed as dist
    if dist.get_backend(group) == 'gloo':
        host = local.detach().cpu()
        parts = [torch.empty_like(host) for _ in range(world)]
        dist.all_gather(parts, host, group=group)
        return torch.cat(parts).to(local.device)
    out = torch.empty((world * local.shape[0],) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out, local.contiguous(), group=group)
    return out


class GPjax_p(ModelAbstr):
    """Full-data GParareal correction (models.py:273-473) on the GPU.

    Same constructor, attributes (thetas, jitters, hyp, fatol/xatol default 1e-4, rng =
    default_rng(45) for the random-restart fallback) and training semantics as the reference;
    the d*9 Nelder-Mead fits of a training round advance together, one batched rows x rows
    factorisation per round (nngp_gpfull_fit).  The -LML arithmetic follows the reference's
    expressions, but the Cholesky's summation order is the GPU's own (LAPACK's blocked order is
    not reproduced): parity is to tolerance and on K (tests/test_gpu_gpfull.py)."""

    def __init__(self, n, N, worker_pool=None, theta=None, jitter=None, fatol=None, xatol=None, **kwargs):
        super().__init__(N=N, **kwargs)
        if theta is None:
            theta = [1, 1]
        theta = np.array(theta)
        self.name = 'GP'
        self.hyp = np.ones((n, theta.shape[0], N))
        self.thetas = [tuple(float(v) for v in theta) for _ in range(n)]
        self.jitters = [None for _ in range(n)]
        self.fatol = 1e-4 if fatol is None else fatol
        self.xatol = 1e-4 if xatol is None else xatol
        self.theta = theta
        self.N = N
        self.n = n
        self.pool = worker_pool
        self.rng = np.random.default_rng(45)
        self.maxfev = 200 * theta.shape[0]
        self.tot_train_t = np.zeros(N)
        self.train_count = np.zeros(N)
        self.k = 0
        self.rounds = []
        # per training call: training rows and the likelihood evaluations its fits made (sum of
        # nfev = the (rows+1)^2 matrices factored), for the measured Cholesky rate (bench.py);
        # sharded over ranks, a call's entry counts every rank's fits (tot_train_t stays this rank's)
        self.call_rows, self.call_evals = [], []
        self._dev = None   # (X [rows][n], alpha [n][rows], coef [n][2]) device tensors
        # multi-GPU (the reference's pool.map over the d*9 fits, models.py:386-392):
        # the torch.distributed group the fits are sharded over by coordinate (Parareal sets it;
        # None = the default group when one is initialised, False = never shard)
        self.process_group = kwargs.get('process_group')
        self.shard_fits = kwargs.get('shard_fits', True)

    def get_times(self):
        out = super().get_times()
        with np.errstate(invalid='ignore', divide='ignore'):
            avg = (self.tot_train_t / self.train_count)[:self.k + 1]
        out.update({'serial_train_time': self.tot_train_t[:self.k + 1], 'avg_serial_train_time': avg})
        return out

    # ---------------------------------------------------------------------------- training
    def _fit_batch(self, X, Y, coords, jitters, theta0):
        """pool.map(_get_opt_par[_rnd], ...) (models.py:404-407, 355-358) as one native call."""
        import torch
        nf = len(coords)
        c = np.ascontiguousarray(coords, dtype=np.int32)
        jx, jp = _lib.host_doubles(jitters)
        t0, tp = _lib.host_doubles(np.asarray(theta0, dtype=float).reshape(nf, 2))
        th = np.empty((nf, 2))
        fv = np.empty(nf)
        ne = np.empty(nf, dtype=np.int32)
        rounds = ctypes.c_int32(0)
        ip = ctypes.POINTER(ctypes.c_int32)
        st = time.time()
        _lib.check(_lib.lib().nngp_gpfull_fit(
            X.data_ptr(), X.shape[0], self.n, Y.data_ptr(), nf, c.ctypes.data_as(ip), jp, tp, float(self.fatol),
            float(self.xatol), self.maxfev, th.ctypes.data_as(_lib._dp), fv.ctypes.data_as(_lib._dp),
            ne.ctypes.data_as(ip), ctypes.byref(rounds), torch.cuda.current_stream().cuda_stream))
        self.tot_train_t[min(self.k, self.N - 1)] += time.time() - st
        self.train_count[min(self.k, self.N - 1)] += nf
        self.rounds.append(int(rounds.value))
        self.call_rows.append(int(X.shape[0]))
        self.call_evals.append(int(ne.astype(np.int64).sum()))
        return th, fv, ne

    def _train_coord_rnd(self, X, Y, coord):
        """models.py:352-374: random restarts for a coordinate whose fits all failed."""
        tot_rnd = max(3, int(self.N / 9))
        ins = list(product([coord for _ in range(tot_rnd)], JITTERS))
        thetas = [10 ** self.rng.uniform(-4, 1, (len(self.theta))) for _ in range(len(ins))]
        th, fv, _ = self._fit_batch(X, Y, [i[0] for i in ins], [i[1] for i in ins], thetas)
        opt_params, opt_fval, opt_jitter = _select_fit(th, fv, np.array([i[1] for i in ins]))
        if np.isinf(opt_fval):
            print('random restart failed')
            opt_params, opt_fval, opt_jitter = self._train_coord_rnd(X, Y, coord)
        return opt_params, opt_fval, opt_jitter

    def _shard(self):
        """(group, world, rank, c0, c1, chunk) of the coordinate split, or None on one rank."""
        if not self.shard_fits:
            return None
        world, rank = _group_world(self.process_group)
        if world <= 1:
            return None
        chunk = (self.n + world - 1) // world
        c0, c1 = min(rank * chunk, self.n), min((rank + 1) * chunk, self.n)
        return self.process_group, world, rank, c0, c1, chunk

    def _train(self, X, Y, old_thetas):
        """models.py:376-417: every (coordinate, jitter) fit from the coordinate's old theta.
        Over several ranks each fits its own contiguous block of coordinates (every fit's
        arithmetic is independent of which others share its batch), then ONE all-gather of
        (theta, fval, nfev) gives every rank all fits; the selection, the random-restart fallback
        (whose draws come from the shared rng stream) and the weights stay replicated."""
        nj = len(JITTERS)
        sh = self._shard()
        if sh is None:
            ins = list(product(range(self.n), JITTERS))
            th, fv, _ = self._fit_batch(X, Y, [i[0] for i in ins], [i[1] for i in ins],
                                        [old_thetas[i[0]] for i in ins])
        else:
            import torch
            group, world, rank, c0, c1, chunk = sh
            buf = torch.zeros((chunk * nj, 4), dtype=torch.float64, device=X.device)
            if c1 > c0:
                ins = list(product(range(c0, c1), JITTERS))
                th_l, fv_l, ne_l = self._fit_batch(X, Y, [i[0] for i in ins], [i[1] for i in ins],
                                                   [old_thetas[i[0]] for i in ins])
                buf[:len(ins)] = torch.tensor(np.column_stack([th_l, fv_l, ne_l]), dtype=torch.float64)
            allf = _gather_rows(buf, group, world).cpu().numpy()[:self.n * nj]
            th, fv = np.ascontiguousarray(allf[:, :2]), np.ascontiguousarray(allf[:, 2])
            self.train_count[min(self.k, self.N - 1)] += self.n * nj - (c1 - c0) * nj   # all fits, as one rank counts them
            # the call's evaluations over ALL ranks' fits (the gathered nfev column), consistent
            # with train_count: bench.py's executed Cholesky rate reads these
            total = int(allf[:, 3].astype(np.int64).sum())
            if c1 > c0:
                self.call_evals[-1] = total
            else:
                self.call_rows.append(int(X.shape[0]))
                self.call_evals.append(total)
        temp = np.zeros((self.n, len(self.theta)))
        nj = len(JITTERS)
        for j in range(self.n):
            sl = slice(j * nj, (j + 1) * nj)
            opt_params, opt_fval, opt_jitter = _select_fit(th[sl], fv[sl], JITTERS)
            if np.isinf(opt_fval):
                print('------> GP trainign failed for coordinate', j)
                opt_params, opt_fval, opt_jitter = self._train_coord_rnd(X, Y, j)
            self.thetas[j] = opt_params
            self.jitters[j] = opt_jitter
            temp[j, :] = opt_params
        return temp

    def _weights(self, X, Y):
        """The posterior weights _predict memoises (models.py:441-453): alpha_j = K_j^-1 y_j for
        the chosen (theta_j, jitter_j).  The reference keys its memo by theta alone, so a
        coordinate whose theta equals an earlier coordinate's reuses that coordinate's weights
        (reproduced)."""
        import torch
        n, rows = self.n, X.shape[0]
        ip = ctypes.POINTER(ctypes.c_int32)

        def lml(c0, c1, alpha_out):
            th, tp = _lib.host_doubles(np.array(self.thetas[c0:c1], dtype=float))
            jx, jp = _lib.host_doubles(np.array(self.jitters[c0:c1], dtype=float))
            c = np.arange(c0, c1, dtype=np.int32)
            fv = np.empty(c1 - c0)
            _lib.check(_lib.lib().nngp_gpfull_lml(
                X.data_ptr(), rows, n, Y.data_ptr(), c1 - c0, c.ctypes.data_as(ip), jp, tp,
                fv.ctypes.data_as(_lib._dp), alpha_out.data_ptr(), torch.cuda.current_stream().cuda_stream))
            return fv

        sh = self._shard()
        if sh is None:
            alpha = torch.empty((n, rows), dtype=torch.float64, device=X.device)
            fv = lml(0, n, alpha)
        else:   # each rank its coordinates' weights, then one all-gather of [chunk][rows] (+ fval)
            group, world, rank, c0, c1, chunk = sh
            buf = torch.zeros((chunk, rows + 1), dtype=torch.float64, device=X.device)
            if c1 > c0:
                part = torch.empty((c1 - c0, rows), dtype=torch.float64, device=X.device)
                fv_l = lml(c0, c1, part)
                buf[:c1 - c0, 1:] = part
                buf[:c1 - c0, 0] = torch.tensor(fv_l, dtype=torch.float64)
            allb = _gather_rows(buf, group, world)[:n]
            alpha = allb[:, 1:].contiguous()
            fv = allb[:, 0].cpu().numpy()
        if np.any(np.isinf(fv)):
            raise np.linalg.LinAlgError('Matrix is not positive definite')   # np.linalg.cholesky in _predict
        first = {}
        for j in range(n):
            key = tuple(self.thetas[j])
            if key in first:
                alpha[j] = alpha[first[key]]
            else:
                first[key] = j
        coef = torch.tensor([[-0.5 * (1 / (sx * sx)), sy * sy] for sx, sy in self.thetas],
                            dtype=torch.float64, device=X.device)
        return alpha, coef

    def fit(self, x, y, k, *args, **kwargs):
        """models.py:420-425."""
        torch = _lib.require_gpu()
        self.k = k
        X, Y = _lib.as_device(x), _lib.as_device(y)
        new_hyp = self._train(X, Y, self.thetas)
        if k + 1 < self.hyp.shape[-1]:
            self.hyp[..., k + 1] = new_hyp
        self.x, self.y = x, y
        alpha, coef = self._weights(X, Y)
        self._dev = (X, alpha, coef)

    # ---------------------------------------------------------------------------- prediction
    def predict_device(self, new_x, out=None, bias=None, stream=None):
        import torch
        X, alpha, coef = self._dev
        if out is None:
            out = torch.empty(self.n, dtype=torch.float64, device=X.device)
        st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().nngp_gpfull_mean(
            X.data_ptr(), X.shape[0], self.n, new_x.data_ptr(), coef.data_ptr(), alpha.data_ptr(),
            bias.data_ptr() if bias is not None else None, out.data_ptr(), st))
        return out

    def predict(self, new_x, prev_F=None, prev_G=None, *args, **kwargs):
        """models.py:456-462 (host arrays in/out)."""
        torch = _lib.require_gpu()
        q = torch.tensor(np.asarray(new_x, dtype=np.float64).reshape(-1), device='cuda')
        return self.predict_device(q).cpu().numpy()

    def store(self):
        new = copy.copy(self)
        new.pool = None
        new._dev = None
        new.hyp = self.hyp[..., :self.k + 3]
        return new

    def state_dict(self):
        st = super().state_dict()
        st['settings'] = {'theta': self.theta.tolist(), 'fatol': self.fatol, 'xatol': self.xatol}
        st.update({'k': self.k, 'thetas': [list(t) for t in self.thetas], 'jitters': self.jitters,
                   'hyp': self.hyp.tolist(), 'tot_train_t': self.tot_train_t.tolist(),
                   'train_count': self.train_count.tolist(), 'rng': self.rng.bit_generator.state})
        return st

    def load_state(self, st):
        super().load_state(st)
        self.k = st['k']
        self.thetas = [tuple(t) for t in st['thetas']]
        self.jitters = list(st['jitters'])
        self.hyp = np.array(st['hyp'], dtype=float)
        self.tot_train_t = np.array(st['tot_train_t'], dtype=float)
        self.train_count = np.array(st['train_count'], dtype=float)
        self.rng.bit_generator.state = st['rng']

    def restore_attrs(self, pool):
        self.pool = pool
        self._dev = None


# ------------------------------------------------------------------------------------------- ELM
ELM_MAX_M, ELM_MAX_RES, ELM_MAX_D = 16, 1024, 8192   # csrc/nngp_elm.h
ELM_SUPPORTED = ("supported: loss='relu', degree 1 or 2, alpha == 0, 1 <= m <= %d, 1 <= res_size <= %d, "
                 '1 <= d <= %d' % (ELM_MAX_M, ELM_MAX_RES, ELM_MAX_D))
_ELM_DEVICE_BYTES = 288e9   # an MI355X's HBM, when no device is visible to ask


def elm_n_poly(d, degree):
    """Columns of sklearn's PolynomialFeatures(degree) on d inputs (models.py:492-494)."""
    return 1 + d + (d * (d + 1) // 2 if degree == 2 else 0)


def _elm_check(d, res_size, loss, alpha, degree, m):
    """Refuse what the GPU ELM does not serve -- before any weights are drawn or GPU work is done."""
    if loss in ('tanh', 'radbad'):
        raise NotImplementedError(f"ELM loss={loss!r}: a bitwise exp / tanh needs a shared polynomial; " + ELM_SUPPORTED)
    if loss != 'relu':
        raise KeyError(loss)   # the reference's losses[loss] (models.py:487-488)
    if degree not in (1, 2):
        raise NotImplementedError(f'ELM degree={degree}; ' + ELM_SUPPORTED)
    if alpha != 0:
        raise NotImplementedError(f'ELM alpha={alpha}; ' + ELM_SUPPORTED)
    if not 1 <= int(m) <= ELM_MAX_M:
        raise ValueError(f'ELM m={m}; ' + ELM_SUPPORTED)
    if not 1 <= int(res_size) <= ELM_MAX_RES:
        raise ValueError(f'ELM res_size={res_size}; ' + ELM_SUPPORTED)
    if not 1 <= int(d) <= ELM_MAX_D:
        raise ValueError(f'ELM d={d}; ' + ELM_SUPPORTED)
    n_poly = elm_n_poly(d, degree)
    nbytes = 8 * int(res_size) * n_poly
    total = _ELM_DEVICE_BYTES
    try:
        import torch
        if torch.cuda.is_available():
            total = torch.cuda.get_device_properties(torch.cuda.current_device()).total_memory
    except ImportError:
        pass
    if nbytes > 0.8 * total:
        raise ValueError(f'ELM weights C = res_size x n_poly = {res_size} x {n_poly} doubles = {nbytes} bytes do not '
                         f'fit the device ({int(total)} bytes, at most 80 % for C)')


class ELM_base():
    """The reference's ELM_base (models.py:476-539) on the GPU: a random-weights network
    relu(bias + C @ PolynomialFeatures(degree)(x)) on the m nearest neighbours, fitted by the
    min-norm interpolation Ridge(alpha=0) computes.  Same constructor, attributes
    (bias [res_size][1], C [res_size][n_poly], drawn from default_rng(seed) in the reference's
    order) and fit / predict / fit_predict on NumPy arrays.  The weights are uploaded once per
    device (C multiplied by R on the host); the hidden features of the training rows are cached on
    the device and only computed for rows appended since the last fit."""

    def __init__(self, d, seed=47, res_size=500, loss='relu', M=1, R=1, alpha=0, degree=2, m=5):
        _elm_check(d, res_size, loss, alpha, degree, m)
        self.d = d
        self.N = res_size
        self.rng = np.random.default_rng(seed)
        self.m = m
        self.loss_name = loss
        self.M = M   # accepted and unused, as in the reference (models.py:522-523)
        self.R = R
        self.alpha = alpha
        self.poly_degree = degree
        self.degree = elm_n_poly(d, degree)   # the reference keeps n_output_features_ here (models.py:494)
        self.bias, self.C = self._init_obj()
        self.x = self.y = None
        self.k = 0
        self._weights = {}    # device index -> (bias [res_size], R * C [res_size][n_poly]) tensors
        self._dev = None      # (X, Y, H, rows): device training set and its hidden rows (H grow-only)

    def _init_obj(self):
        """models.py:500-504."""
        N, rng = self.N, self.rng
        bias = rng.uniform(-1, 1, (N, 1))
        C = rng.uniform(-1, 1, (N, self.degree))
        return bias, C

    # ---------------------------------------------------------------------------- device path
    def weights_device(self, device):
        import torch
        key = torch.device(device).index
        if key not in self._weights:
            try:
                self._weights[key] = (torch.tensor(np.ascontiguousarray(self.bias[:, 0]), device=device),
                                      torch.tensor(np.ascontiguousarray(self.R * self.C), device=device))
            except torch.cuda.OutOfMemoryError as e:
                raise ValueError(f'ELM weights C = {self.N} x {self.degree} doubles = {8 * self.N * self.degree} '
                                 f'bytes do not fit the device') from e
        return self._weights[key]

    def hidden_device(self, X, out=None, stream=None):
        """Hidden rows of the device rows X [rows][d] (nngp_elm_hidden)."""
        import torch
        bias, C = self.weights_device(X.device)
        if out is None:
            out = torch.empty((X.shape[0], self.N), dtype=torch.float64, device=X.device)
        st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().nngp_elm_hidden(X.data_ptr(), X.shape[0], self.d, self.poly_degree, self.N,
                                              bias.data_ptr(), C.data_ptr(), out.data_ptr(), st))
        return out

    def fit_device(self, X, Y):
        """The driver's device-resident training set (torch tensors [rows][d], append-only between
        calls: rows the cache already holds are not read again).  H grows by doubling, so steady-state
        fits allocate nothing."""
        import torch
        rows = int(X.shape[0])
        n0, H = 0, None
        if self._dev is not None and self._dev[0].device == X.device and rows >= self._dev[3]:
            H, n0 = self._dev[2], self._dev[3]
        if H is None or H.shape[0] < rows:
            grown = torch.empty((max(rows, 2 * (H.shape[0] if H is not None else 32)), self.N),
                                dtype=torch.float64, device=X.device)
            if n0:
                grown[:n0] = H[:n0]
            H = grown
        if rows > n0:
            self.hidden_device(X[n0:rows], out=H[n0:rows])
        self._dev = (X, Y, H, rows)
        self.x = self.y = None   # host copies are made on demand (training_set)

    def device_state(self):
        """(X, Y, H, rows) on the device, uploading a host training set given to fit()."""
        if self._dev is None:
            if self.x is None or self.y is None:
                raise AttributeError("'ELM_base' has no training set yet: call fit(x, y, k) first")
            x, y = self.x, self.y
            self.fit_device(_lib.as_device(x), _lib.as_device(y))
            self.x, self.y = x, y
        return self._dev

    def training_set(self):
        """Host (x, y)."""
        if self.x is None and self._dev is not None:
            X, Y, _, rows = self._dev
            return X[:rows].detach().cpu().numpy(), Y[:rows].detach().cpu().numpy()
        return self.x, self.y

    def predict_device(self, new_x, out=None, bias=None, preds=None, stream=None):
        """One correction on device tensors (nngp_elm_predict): preds and / or out = preds + bias."""
        import torch
        X, Y, H, rows = self.device_state()
        b, C = self.weights_device(X.device)
        if preds is None and (out is None or bias is None):
            preds = torch.empty(self.d, dtype=torch.float64, device=X.device)
        st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        ptr = lambda a: a.data_ptr() if a is not None else None
        _lib.check(_lib.lib().nngp_elm_predict(
            X.data_ptr(), Y.data_ptr(), H.data_ptr(), rows, self.d, new_x.data_ptr(), min(int(self.m), rows),
            self.poly_degree, self.N, b.data_ptr(), C.data_ptr(), ptr(preds), ptr(bias), ptr(out), st))
        return preds

    # ------------------------------------------------------------------------- reference API
    def fit(self, x, y, k):
        """models.py:515-518."""
        if hasattr(x, 'data_ptr'):
            self.fit_device(x, y)
        else:
            self.x, self.y = x, y
            self._dev = None
        self.k = k

    def predict(self, new_x):
        """models.py:521-535 (host arrays in, the [d] predicted correction out)."""
        torch = _lib.require_gpu()
        q = torch.tensor(np.asarray(new_x, dtype=np.float64).reshape(-1), device='cuda')
        return self.predict_device(q).cpu().numpy()

    def fit_predict(self, x, y, new_x, k):
        self.fit(x, y, k)
        return self.predict(new_x)


class ELM(ModelAbstr):
    """The RandNet-Parareal correction model (models.py:542-554): ELM_base behind the plugin
    surface, with the driver's device-resident training set and the native sweep."""

    def __init__(self, d, N, seed=47, res_size=20, loss='relu', M=1, R=1, alpha=0, degree=2, m=4, **kwargs):
        super().__init__(N=N, **kwargs)
        self.settings = dict(seed=seed, res_size=res_size, loss=loss, M=M, R=R, alpha=alpha, degree=degree, m=m)
        self.ELM = ELM_base(d=d, **self.settings)
        self.name = 'ELM'
        self.n = d

    def fit(self, x, y, k, *args, **kwargs):
        self.ELM.fit(x, y, k)

    def predict(self, new_x, *args, **kwargs):
        return self.ELM.predict(new_x)

    def predict_device(self, new_x, out=None, bias=None, preds=None, stream=None):
        return self.ELM.predict_device(new_x, out=out, bias=bias, preds=preds, stream=stream)

    x = property(lambda self: self.ELM.training_set()[0])
    y = property(lambda self: self.ELM.training_set()[1])

    def store(self):
        """A deep copy for the result dict: host x / y, no device tensors."""
        e = self.ELM
        x, y = e.training_set()
        saved = (e._dev, e._weights, e.x, e.y)
        e._dev, e._weights, e.x, e.y = None, {}, x, y
        try:
            new = super().store()
        finally:
            e._dev, e._weights, e.x, e.y = saved
        return new

    def state_dict(self):
        """The ELM state of a checkpoint is its constructor arguments (the weights follow from the
        seed); the training set is the checkpoint's x / D."""
        st = super().state_dict()
        st['settings'] = dict(self.settings)
        return st


# ------------------------------------------------------------------------------------------ k-NN
KNN_MAX_COUNTS = 16   # counts one nngp_knn_mean launch serves (include/nngp.h)


def _nn_count(nn):
    """The neighbour count of the k-NN model: an integer in 1..MAX_NEIGHBOURS."""
    if isinstance(nn, str) or isinstance(nn, bool) or not isinstance(nn, (int, np.integer)):
        raise ValueError(f"nn={nn!r}: the k-NN correction takes an integer neighbour count "
                         f"(1..{MAX_NEIGHBOURS}); 'adaptive' is a mode of NNGP_p only")
    if nn < 1:
        raise ValueError(f'nn={nn}: the k-NN correction needs nn >= 1')
    if nn > MAX_NEIGHBOURS:
        raise ValueError(f'nn={nn}: the GPU k-NN correction supports at most {MAX_NEIGHBOURS} neighbours')
    return int(nn)


def _knn_tensor(t, name, shape, device, dtype=None):
    """A device tensor handed to nngp_knn_mean by address: it must be what the kernel reads it as."""
    import torch
    dtype = torch.float64 if dtype is None else dtype
    if not torch.is_tensor(t) or t.dtype != dtype or t.device != device or tuple(t.shape) != tuple(shape) \
            or not t.is_contiguous():
        what = f'{tuple(t.shape)} {t.dtype} on {t.device}' + ('' if t.is_contiguous() else ', not contiguous') \
            if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f'{name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device} (got {what})')
    return t.data_ptr()


class NN(ModelAbstr):
    """k-NN Parareal (Figure_2.py:455-475): the correction is the plain average of the nn nearest
    neighbours' F - G rows, on the GPU (nngp_knn_mean).  Same constructor
    (NN(N=..., nn=10)) and name (f'{nn}-NN') as the reference."""

    def __init__(self, *args, **kwargs):
        self.nn = _nn_count(kwargs.get('nn', 10))
        self.name = f'{self.nn}-NN'
        super().__init__(*args, **kwargs)
        self.k = 0
        self._dev_xy = None
        self._host_xy = None

    def fit(self, x, y, k, *args, **kwargs):
        """Figure_2.py:461-465; a device-resident training set (torch tensors) is kept as it is."""
        self.k = k
        if hasattr(x, 'data_ptr'):
            self._dev_xy, self._host_xy = (x, y), None
        else:
            self._dev_xy, self._host_xy = None, (x, y)

    def _host(self):
        if self._host_xy is None:
            if self._dev_xy is None:
                raise AttributeError("'NN' has no training set yet: call fit(x, y, k) first")
            self._host_xy = tuple(v.detach().cpu().numpy() for v in self._dev_xy)
        return self._host_xy

    x = property(lambda self: self._host()[0])
    y = property(lambda self: self._host()[1])

    def device_xy(self):
        """(X, Y) on the device, uploading a host training set given to fit()."""
        if self._dev_xy is None:
            if self._host_xy is None:
                raise AttributeError("'NN' has no training set yet: call fit(x, y, k) first")
            self._dev_xy = (_lib.as_device(self._host_xy[0]), _lib.as_device(self._host_xy[1]))
        X, Y = self._dev_xy
        if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError(f'the training set must be [rows >= 1][d >= 1] (got x of shape {tuple(X.shape)})')
        _knn_tensor(X, 'x', X.shape, X.device)
        _knn_tensor(Y, 'y', X.shape, X.device)
        return self._dev_xy

    # ---------------------------------------------------------------------------- device path
    def predict_batch_device(self, Q, counts=None, out=None, idx_out=None, stream=None):
        """The means of the counts[j] nearest rows for every row of Q [n_q][d], one launch set
        (nngp_knn_mean): out [len(counts)][n_q][d].  counts defaults to [nn]; each is clamped to the
        number of training rows (argsort(...)[:nn] on fewer rows keeps them all)."""
        import torch
        X, Y = self.device_xy()
        rows, d = int(X.shape[0]), int(X.shape[1])
        counts = [self.nn] if counts is None else [_nn_count(c) for c in counts]
        if not 1 <= len(counts) <= KNN_MAX_COUNTS:
            raise ValueError(f'{len(counts)} counts: one launch serves 1..{KNN_MAX_COUNTS}')
        cm = np.array([min(c, rows) for c in counts], dtype=np.int32)
        if not torch.is_tensor(Q) or Q.dim() != 2:
            raise ValueError('Q must be a device tensor of shape [n_q][d]')
        n_q = int(Q.shape[0])
        q_ptr = _knn_tensor(Q, 'Q', (n_q, d), X.device)
        if out is None:
            out = torch.empty((len(cm), n_q, d), dtype=torch.float64, device=X.device)
        out_ptr = _knn_tensor(out, 'out', (len(cm), n_q, d), X.device)
        idx_ptr = None if idx_out is None else _knn_tensor(idx_out, 'idx_out', (n_q, int(cm.max())), X.device,
                                                           torch.int32)
        st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().nngp_knn_mean(
            X.data_ptr(), Y.data_ptr(), rows, d, q_ptr, n_q, cm.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            len(cm), out_ptr, idx_ptr, None, None, st))
        return out

    def predict_device(self, new_x, out=None, bias=None, preds=None, stream=None):
        """One correction on device tensors: preds, and out = preds + bias when both are given."""
        import torch
        X, Y = self.device_xy()
        rows, d = int(X.shape[0]), int(X.shape[1])
        if preds is None:
            preds = torch.empty(d, dtype=torch.float64, device=X.device)
        if (out is None) != (bias is None):
            raise ValueError('out and bias go together')
        cm = (ctypes.c_int32 * 1)(min(self.nn, rows))
        ptr = lambda t, name: None if t is None else _knn_tensor(t, name, (d,), X.device)
        st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().nngp_knn_mean(
            X.data_ptr(), Y.data_ptr(), rows, d, ptr(new_x, 'new_x'), 1, cm, 1, ptr(preds, 'preds'), None,
            ptr(bias, 'bias'), ptr(out, 'out'), st))
        return preds

    # ------------------------------------------------------------------------- reference API
    def predict(self, new_x, prev_F=None, prev_G=None, *args, **kwargs):
        """Figure_2.py:467-475 (host arrays in, the [d] mean out)."""
        torch = _lib.require_gpu()
        q = torch.tensor(np.asarray(new_x, dtype=np.float64).reshape(-1), device='cuda')
        return self.predict_device(q).cpu().numpy()

    def store(self):
        """A deep copy for the result dict: host x / y, no device tensors."""
        if self._dev_xy is not None:
            self._host()
        dev, self._dev_xy = self._dev_xy, None
        try:
            new = super().store()
        finally:
            self._dev_xy = dev
        return new

    def state_dict(self):
        st = super().state_dict()
        st['settings'] = {'nn': self.nn}
        st['k'] = self.k
        return st

    def load_state(self, st):
        super().load_state(st)
        self.k = st['k']
