"""Propagators -- the reference's SolverAbstr / SolverRK plugin surface (solver.py:21-113) with a
HIP backend.

Single-slice calls (`run_F(t0, t1, u0)`, `run_G`, their `_timed` variants) keep the reference's
signatures and numpy in/out.  The Parareal driver uses the batched device entry points
`run_F_batch` / `run_G_batch`, which integrate every slice of one iteration in ONE kernel launch
(nngp_rk_batch); that replaces `pool.map(solver.run_F_timed, ...)` at parareal.py:310-315.
`run_F_traj_batch` / `run_G_traj_batch` return every slice's sampled trajectory from one launch
(nngp_rk_traj); `run_F_full` / `run_G_full` (RK.run, numpy in/out) are built on it.

Step conventions (include/nngp.h):
  step_mode='fixed'    (default)  h = (t1-t0)/steps            RK.run_get_last, RK.py:101-109
  step_mode='linspace'            h_n = t[n+1]-t[n] of np.linspace  legacy new_lib.RK, RK.py:91-99
`thresh` reproduces the paging of SolverRK._run_RK_paged (solver.py:86-99) including its quirk
(each page re-uses the full steps-1 count over 1/n_pages of the slice).
`fma=True` (opt-in; env NNGP_RK_CONTRACT=1 flips the default) runs F and G on the contracted code
object (NNGP_STEP_CONTRACT): a*b+c fused, ~25 % fewer fp64 instructions per step, end states within
1e-12 relative of the exact build instead of bitwise (tests/test_gpu_contract.py).

`SolverScipy` (solver.py:116-148) is the adaptive fine propagator: scipy's RK23 / RK45 step-size
control with max_step = (t1-t0)/Nf, every slice in one launch (nngp_rk_adaptive), G through the
fixed-step SolverRK it derives from.
"""
import os
import ctypes
import time

import numpy as np

from . import _lib


def calc_time(f):
    def wrapper(*args, **kwargs):
        s_time = time.time()
        ret = f(*args, **kwargs)
        return ret, time.time() - s_time
    return wrapper


class SolverAbstr:
    """Abstract propagator: run_*(t0, t1, u0) returns the solution at t1 (solver.py:29-69)."""

    def run_F(self, t0, t1, u0):
        raise NotImplementedError('run_F not implemented')

    @calc_time
    def run_F_timed(self, t0, t1, u0):
        return self.run_F(t0, t1, u0)

    def run_F_full(self, t0, t1, u0):
        raise NotImplementedError('run_F_full not implemented')

    @calc_time
    def run_F_full_timed(self, t0, t1, u0):
        return self.run_F_full(t0, t1, u0)

    def run_G(self, t0, t1, u0):
        raise NotImplementedError('run_G not implemented')

    @calc_time
    def run_G_timed(self, t0, t1, u0):
        return self.run_G(t0, t1, u0)

    def run_G_full(self, t0, t1, u0):
        raise NotImplementedError('run_G_full not implemented')

    @calc_time
    def run_G_full_timed(self, t0, t1, u0):
        return self.run_G_full(t0, t1, u0)


def _paging_schedule(steps, thresh):
    """solver.py:91-93: the page lengths (in units of step) and the per-page step count."""
    steps = steps - 1
    n_full = int(steps / thresh)
    rem = steps % thresh
    return [thresh] * n_full + [rem] * int(rem != 0), steps


class SolverRK(SolverAbstr):
    """Fixed-step explicit RK fine (F) and coarse (G) propagators on the GPU.

    f: the VectorField returned by ODE.get_vector_field() (carries the device descriptor).
    Ng, Nf: steps per slice (modern convention, configs.py); F, G: 'RK1'|'RK2'|'RK4'|'RK8'.
    """

    def __init__(self, f, Ng, Nf, F, G, thresh=1e7, use_jax=True, step_mode='fixed', fma=None, **kwargs):
        if not hasattr(f, 'csystem'):
            raise TypeError('f must be the VectorField returned by ODE.get_vector_field()')
        self.f = f
        self.Ng = int(Ng)
        self.Nf = int(Nf)
        self.F = F
        self.G = G
        self.thresh = thresh
        if F not in _lib.TABLEAU or G not in _lib.TABLEAU:
            raise NotImplementedError('Only RK1, RK2, RK4 and RK8 are implemented')
        self.step_mode = {'fixed': _lib.STEP_FIXED, 'linspace': _lib.STEP_LINSPACE}[step_mode]
        if fma is None:
            fma = os.environ.get('NNGP_RK_CONTRACT') == '1'
        self.fma = bool(fma)
        if self.fma:
            self.step_mode |= _lib.STEP_CONTRACT

    # -------------------------------------------------------------------------------- device
    def _launch(self, method, t0, t1, steps, U0, out, stream):
        import torch
        cs = self.f.csystem(U0.device)
        st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().nngp_rk_batch(ctypes.byref(cs), _lib.TABLEAU[method], self.step_mode,
                                             U0.shape[0], t0.data_ptr(), t1.data_ptr(), int(steps),
                                             U0.data_ptr(), out.data_ptr(), st))
        return out

    def _run_batch(self, method, steps, t0, t1, U0, out=None, stream=None):
        """Integrate U0[i] from t0[i] to t1[i] for all i (one launch per page)."""
        import torch
        if out is None:
            out = torch.empty_like(U0)
        n = U0.shape[0]
        if n == 0:
            return out
        assert U0.dtype == torch.float64 and U0.is_contiguous() and U0.is_cuda
        if steps > self.thresh:   # paged quirk, solver.py:86-99 -- rare; host-side schedule
            t0h = t0.detach().cpu().numpy() if torch.is_tensor(t0) else np.asarray(t0, dtype=float)
            t1h = t1.detach().cpu().numpy() if torch.is_tensor(t1) else np.asarray(t1, dtype=float)
            iters, psteps = _paging_schedule(steps, self.thresh)
            step = (t1h - t0h) / psteps
            cur = U0
            a = t0h.copy()
            for temp_steps in iters:
                b = a + step * temp_steps
                ta = torch.tensor(a, dtype=torch.float64, device=U0.device)
                tb = torch.tensor(b, dtype=torch.float64, device=U0.device)
                self._launch(method, ta, tb, psteps, cur, out, stream)
                cur = out
                a = b
            return out
        if not torch.is_tensor(t0):
            t0 = torch.tensor(np.asarray(t0, dtype=float), device=U0.device)
            t1 = torch.tensor(np.asarray(t1, dtype=float), device=U0.device)
        return self._launch(method, t0, t1, steps, U0, out, stream)

    def coarse_is_paged(self):
        return self.Ng > self.thresh

    def initial_coarse(self, t_dev, UG, N):
        """Initial coarse sweep (parareal.py:265-270): UG[i+1] = G(t[i], t[i+1], UG[i]), one
        slice after the other."""
        for i in range(N):
            self.run_G_batch(t_dev[i:i + 1], t_dev[i + 1:i + 2], UG[i:i + 1], out=UG[i + 1:i + 2])

    def run_F_batch(self, t0, t1, U0, out=None, stream=None):
        return self._run_batch(self.F, self.Nf, t0, t1, U0, out, stream)

    def run_G_batch(self, t0, t1, U0, out=None, stream=None):
        return self._run_batch(self.G, self.Ng, t0, t1, U0, out, stream)

    # -------------------------------------------------------------------------- reference API
    def _single(self, method, steps, t0, t1, u0):
        torch = _lib.require_gpu()
        U0 = torch.tensor(np.asarray(u0, dtype=np.float64).reshape(1, -1), device='cuda')
        out = self._run_batch(method, steps, np.array([t0], dtype=float), np.array([t1], dtype=float), U0)
        return out[0].cpu().numpy()

    def run_F(self, t0, t1, u0):
        return self._single(self.F, self.Nf, t0, t1, u0)

    def run_G(self, t0, t1, u0):
        return self._single(self.G, self.Ng, t0, t1, u0)

    # -------------------------------------------------------------------------- trajectories
    @staticmethod
    def traj_rows(steps, every):
        """Rows of a sampled trajectory: the start, every `every`-th step, and the last step."""
        steps, every = int(steps), int(every)
        return 1 + -(-steps // every)

    @staticmethod
    def traj_times(t0, t1, steps, every):
        """Time stamps of a sampled trajectory's rows: np.linspace(t0, t1, steps + 1) (RK.run,
        RK.py:91-99) at the step counts 0, every, 2*every, ..., steps."""
        steps, every = int(steps), int(every)
        idx = np.minimum(np.arange(SolverRK.traj_rows(steps, every)) * every, steps)
        return np.linspace(t0, t1, num=steps + 1)[idx]

    def _traj_batch(self, method, steps, t0, t1, U0, every, out, stream, step_mode=None):
        """Every slice's sampled trajectory in ONE launch (nngp_rk_traj): out[i, p] is the state of
        slice i after min(p*every, steps) steps from U0[i], out[i, 0] = U0[i]."""
        import torch
        steps, every = int(steps), int(every)
        if every < 1:
            raise ValueError(f'every must be >= 1 (got {every})')
        n, d = U0.shape
        n_out = self.traj_rows(steps, every)
        if out is None:
            out = torch.empty((n, n_out, d), dtype=torch.float64, device=U0.device)
        assert tuple(out.shape) == (n, n_out, d) and out.dtype == torch.float64 and out.is_contiguous()
        if n == 0:
            return out
        assert U0.dtype == torch.float64 and U0.is_contiguous() and U0.is_cuda and out.is_cuda
        if not torch.is_tensor(t0):
            t0 = torch.tensor(np.asarray(t0, dtype=float), device=U0.device)
            t1 = torch.tensor(np.asarray(t1, dtype=float), device=U0.device)
        cs = self.f.csystem(U0.device)
        st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        mode = self.step_mode if step_mode is None else step_mode
        _lib.check(_lib.lib().nngp_rk_traj(ctypes.byref(cs), _lib.TABLEAU[method], mode, n, t0.data_ptr(),
                                            t1.data_ptr(), steps, every, U0.data_ptr(), out.data_ptr(), st))
        return out

    def _traj_mode(self, step_mode):
        if step_mode is None:
            return None
        return ({'fixed': _lib.STEP_FIXED, 'linspace': _lib.STEP_LINSPACE}[step_mode] |
                (self.step_mode & _lib.STEP_CONTRACT))

    def run_F_traj_batch(self, t0, t1, U0, every=1, out=None, stream=None, step_mode=None):
        """(n, d) device states -> (n, traj_rows(Nf, every), d) device trajectories of the fine
        solver in one launch, in the solver's own step_mode and fma: with 'fixed' steps the last
        row is bitwise run_F_batch's end state.  step_mode='linspace' walks np.linspace(t0, t1,
        Nf + 1) instead, as RK.run does (run_F_full, Parareal.build_cont_traj)."""
        return self._traj_batch(self.F, self.Nf, t0, t1, U0, every, out, stream, self._traj_mode(step_mode))

    def run_G_traj_batch(self, t0, t1, U0, every=1, out=None, stream=None, step_mode=None):
        return self._traj_batch(self.G, self.Ng, t0, t1, U0, every, out, stream, self._traj_mode(step_mode))

    def _full(self, method, steps, t0, t1, u0, every=1):
        """Trajectory on the np.linspace grid (RK.run, RK.py:91-99), every `every`-th point of it:
        one launch in LINSPACE mode, whose step n is h = t[n+1] - t[n] of that grid."""
        torch = _lib.require_gpu()
        U0 = torch.tensor(np.asarray(u0, dtype=np.float64).reshape(1, -1), device='cuda')
        out = self._traj_batch(method, steps, np.array([t0], dtype=float), np.array([t1], dtype=float), U0, every,
                               None, None, self._traj_mode('linspace'))
        return out[0].cpu().numpy()

    def run_F_full(self, t0, t1, u0, every=1):
        return self._full(self.F, self.Nf, t0, t1, u0, every)

    def run_G_full(self, t0, t1, u0, every=1):
        return self._full(self.G, self.Ng, t0, t1, u0, every)


class SolverScipy(SolverRK):
    """The reference's adaptive fine propagator (solver.py:116-148): F is scipy's RK23 or RK45 with
    max_step = (t1-t0)/Nf per slice, every slice of an iteration in ONE launch (nngp_rk_adaptive);
    G is the fixed-step SolverRK it is derived from, as the reference's inner `rk_solver`.

    F: 'RK45' / 'RK4', 'RK23' / 'RK2' (solver.py:130-135).  kwargs are those the reference forwards
    to solve_ivp: rtol (1e-3), atol (1e-6), both scalars, and first_step (None: selected as scipy
    does); plus max_attempts, the cap on attempted steps per slice (100*Nf + 1000).  The arithmetic
    is the fixed operation order of DESIGN.md 3.2d (tests/adaptive_ref.py), not scipy's BLAS and
    libm one; only the exact build is offered (no fma).  After every launch `last_stats` holds the
    per-slice 'status', 'nfev', 'n_accepted' and 'n_rejected' as numpy arrays (the reference's
    "did x more steps" print fires on every RK45 call by construction and is dropped).
    """

    _MAP = {'RK2': 'RK23', 'RK4': 'RK45', 'RK8': 'DOP853'}   # solver.py:131
    _WHY = {1: 'the required step size fell below the spacing between numbers (min_step)',
            2: 'max_attempts attempted steps were reached'}

    def __init__(self, f, Ng, Nf, G, F='RK45', use_jax=True, **kwargs):
        kwargs = dict(kwargs)
        if kwargs.pop('fma', None) or os.environ.get('NNGP_RK_CONTRACT') == '1':
            raise NotImplementedError('SolverScipy has no contracted build: fma=True / NNGP_RK_CONTRACT=1 is not '
                                      'offered with the adaptive propagator')
        method = self._map_solver(F)
        if method not in _lib.ADAPTIVE:
            raise NotImplementedError(f'SolverScipy: method {method!r} is not implemented (only RK23 and RK45)')
        rtol = kwargs.pop('rtol', 1e-3)
        atol = kwargs.pop('atol', 1e-6)
        first_step = kwargs.pop('first_step', None)
        max_attempts = kwargs.pop('max_attempts', None)
        if kwargs:
            raise TypeError(f'SolverScipy: keyword {sorted(kwargs)[0]!r} is not supported (rtol, atol, first_step, '
                            'max_attempts)')
        for name, v in (('rtol', rtol), ('atol', atol)):
            if np.ndim(v) != 0:
                raise TypeError(f'SolverScipy: {name} must be a scalar (an array {name} is not supported)')
        rtol, atol = float(rtol), float(atol)
        if not (np.isfinite(rtol) and rtol > 0):
            raise ValueError(f'SolverScipy: rtol must be positive and finite (got {rtol})')
        if not (np.isfinite(atol) and atol >= 0):
            raise ValueError(f'SolverScipy: atol must be non-negative and finite (got {atol})')
        eps100 = 100 * np.finfo(float).eps
        if rtol < eps100:   # scipy's validate_tol
            import warnings
            warnings.warn(f'At least one element of `rtol` is too small. Setting `rtol = np.maximum(rtol, {eps100})`.',
                          stacklevel=2)
            rtol = eps100
        if first_step is not None:
            if np.ndim(first_step) != 0:
                raise TypeError('SolverScipy: first_step must be a scalar')
            first_step = float(first_step)
            if not (np.isfinite(first_step) and first_step > 0):   # validate_first_step
                raise ValueError('SolverScipy: `first_step` must be positive.')
        super().__init__(f, Ng, Nf, F=G, G=G, fma=False)
        self.F = method
        if max_attempts is None:
            max_attempts = 100 * self.Nf + 1000
        if int(max_attempts) != max_attempts or int(max_attempts) < 1:
            raise ValueError(f'SolverScipy: max_attempts must be an integer >= 1 (got {max_attempts})')
        self.rtol, self.atol, self.first_step, self.max_attempts = rtol, atol, first_step, int(max_attempts)
        self.kwargs = dict(rtol=rtol, atol=atol, first_step=first_step)
        self.last_stats = None

    def _map_solver(self, solver):
        return self._MAP.get(solver, solver)

    def run_F_batch(self, t0, t1, U0, out=None, stream=None):
        """Integrate U0[i] from t0[i] to t1[i] for all i in one launch, then read the per-slice
        status back (one small device-to-host copy) and raise NNGPError for the first slice that
        did not reach t1."""
        import torch
        if out is None:
            out = torch.empty_like(U0)
        n = U0.shape[0]
        if n == 0:
            z = np.zeros(0, dtype=np.int64)
            self.last_stats = dict(status=z, nfev=z.copy(), n_accepted=z.copy(), n_rejected=z.copy())
            return out
        assert U0.dtype == torch.float64 and U0.is_contiguous() and U0.is_cuda
        if not torch.is_tensor(t0):
            t0 = torch.tensor(np.asarray(t0, dtype=float), device=U0.device)
            t1 = torch.tensor(np.asarray(t1, dtype=float), device=U0.device)
        if self.first_step is not None and self.first_step > float((t1 - t0).abs().min()):   # validate_first_step
            raise ValueError('SolverScipy: `first_step` exceeds bounds.')
        cs = self.f.csystem(U0.device)
        stats = torch.empty((n, 4), dtype=torch.int64, device=U0.device)
        st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().nngp_rk_adaptive(ctypes.byref(cs), _lib.ADAPTIVE[self.F], n, t0.data_ptr(), t1.data_ptr(),
                                               self.Nf, self.rtol, self.atol, self.first_step or 0.0,
                                               self.max_attempts, U0.data_ptr(), out.data_ptr(), stats.data_ptr(), st))
        if stream is not None:   # the copy below must follow the launch on the caller's stream
            with torch.cuda.stream(torch.cuda.ExternalStream(stream)):
                h = stats.cpu().numpy()
        else:
            h = stats.cpu().numpy()
        self.last_stats = dict(status=h[:, 0].copy(), nfev=h[:, 1].copy(), n_accepted=h[:, 2].copy(),
                               n_rejected=h[:, 3].copy())
        bad = np.flatnonzero(h[:, 0])
        if bad.size:
            i = int(bad[0])
            raise _lib.NNGPError(f'SolverScipy ({self.F}): slice {i} of {n} failed with status {int(h[i, 0])}: '
                                 f'{self._WHY.get(int(h[i, 0]), "unknown status")} after {int(h[i, 2])} accepted and '
                                 f'{int(h[i, 3])} rejected steps ({bad.size} failing slice(s) in this launch)')
        return out

    def run_F(self, t0, t1, u0):
        torch = _lib.require_gpu()
        U0 = torch.tensor(np.asarray(u0, dtype=np.float64).reshape(1, -1), device='cuda')
        return self.run_F_batch(np.array([t0], dtype=float), np.array([t1], dtype=float), U0)[0].cpu().numpy()

    # the reference's SolverScipy has no run_F_full either (solver.py:116-148)
    def run_F_traj_batch(self, *args, **kwargs):
        raise NotImplementedError('SolverScipy has no sampled fine trajectory (run_F_traj_batch, run_F_full, '
                                  'Parareal.build_cont_traj): the adaptive propagator has no dense output')

    def run_F_full(self, t0, t1, u0, every=1):
        return self.run_F_traj_batch()
