"""ODE / PDE systems -- same classes, constructor arguments, bounds and initial conditions as the
reference's systems.py (modern API).  The right-hand side itself is evaluated on the GPU inside
the HIP propagator (csrc/nngp_rk.hip); `get_vector_field()` returns a `VectorField` that
carries the device descriptor (struct nngp_system) and, when called as f(t, u), evaluates the
RHS on the GPU through nngp_rhs_batch.

Reference: /root/reference/systems.py (ODE 23-77, FHN_ODE 80-106, Rossler 109-137, Hopf 140-172,
DblPend 175-199, Brusselator 202-222, Lorenz 225-247, ThomasLabyrinth 250-288, FHN_PDE 291-398,
Burgers 402-459, DiffReact 463-577): all ten of the reference's systems.
"""
import ctypes

import numpy as np

from . import _lib
from .utils import Normalize


class VectorField:
    """Device-side vector field f_n(t, u) = f(inverse(u)) * scale (systems.py:32-44)."""

    def __init__(self, ode):
        self.ode = ode
        self._dev = {}

    def csystem(self, device):
        """struct nngp_system for `device` (norm table uploaded once and kept alive)."""
        import torch
        key = str(device)
        if key not in self._dev:
            ode = self.ode
            table = ode.normalizer.device_table(ode.d) if ode.normalized else None
            norm_t = None
            if table is not None:
                norm_t = torch.tensor(table, dtype=torch.float64, device=device)
            p = (ctypes.c_double * 4)(*(list(ode.param) + [0.0] * (4 - len(ode.param))))
            cs = _lib.CSystem(ode.kind, ode.d, ode.nx, int(ode.normalized), p,
                              norm_t.data_ptr() if norm_t is not None else None)
            cs._keep_alive = norm_t   # the struct holds a raw device pointer into this tensor
            self._dev[key] = (cs, norm_t)
        return self._dev[key][0]

    def __call__(self, t, u):
        torch = _lib.require_gpu()
        u = np.asarray(u, dtype=np.float64)
        single = u.ndim == 1
        U = torch.tensor(np.atleast_2d(u), dtype=torch.float64, device='cuda')
        out = torch.empty_like(U)
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().nngp_rhs_batch(ctypes.byref(self.csystem(U.device)), U.shape[0],
                                              U.data_ptr(), out.data_ptr(), st))
        r = out.cpu().numpy()
        return r[0] if single else r


class ODE():
    kind = None
    nx = 0

    def __init__(self, name, mn, mx, u0, normalization=None, use_jax=True, param=()):
        self.name = name
        self.normalizer = Normalize(mn, mx, normalization)
        self.normalized = self.normalizer.norm_type == '-11'
        self.u0 = self.normalizer.fit(u0)
        self.use_jax = use_jax       # accepted for signature compatibility; unused
        self.d = int(np.asarray(u0).shape[0])
        self.param = tuple(param)

    def get_vector_field(self):
        return VectorField(self)

    def set_default_init_cond(self, u0):
        self.u0 = self.normalizer.fit(u0)

    def get_init_cond(self, *args, u0=None, **kwargs):
        if u0 is None:
            u0 = self.u0
        else:
            u0 = self.normalizer.fit(u0)
        return np.array(u0, dtype=float)

    def get_dim(self):
        return self.u0.shape[0]


class FHN_ODE(ODE):
    kind = _lib.SYS_FHN_ODE

    def __init__(self, **kwargs):
        mn, mx = np.array([[-2, -1], [2.1, 1.2]])
        super().__init__('FHN_ODE', mn, mx, np.array([-1, 1]), **kwargs)


class Rossler(ODE):
    kind = _lib.SYS_ROSSLER

    def __init__(self, **kwargs):
        mn, mx = np.array([[-10, -11, 0], [12, 8, 23]])
        super().__init__('Rossler', mn, mx, np.array([0, -6.78, 0.02]), **kwargs)


class Hopf(ODE):
    kind = _lib.SYS_HOPF

    def __init__(self, tspan=[-20, 500], **kwargs):
        mn, mx = np.array([[-23, -23, 0], [23, 23, 1]])
        u0 = np.array([0.1, 0.1, tspan[0]])
        self.maxtime = tspan[1]
        super().__init__('Hopf', mn, mx, u0, param=(float(tspan[1]),), **kwargs)


class DblPend(ODE):
    kind = _lib.SYS_DBL_PEND

    def __init__(self, **kwargs):
        mn, mx = np.array([[-2, -2.5, -17, -3.5], [2, 2.5, 1, 3.5]])
        super().__init__('DblPend', mn, mx, np.array([-0.5, 0, 0, 0]), **kwargs)


class Brusselator(ODE):
    kind = _lib.SYS_BRUSSELATOR

    def __init__(self, **kwargs):
        mn, mx = np.array([[0.4, 0.9], [4, 5]])
        super().__init__('Brusselator', mn, mx, np.array([1, 3.07]), **kwargs)


class Lorenz(ODE):
    kind = _lib.SYS_LORENZ

    def __init__(self, **kwargs):
        mn, mx = np.array([[-17.1, -23, 6], [18.1, 25, 45]])
        super().__init__('Lorenz', mn, mx, np.array([-15, -15, 20]), **kwargs)


class ThomasLabyrinth(ODE):
    kind = _lib.SYS_THOMAS_LABYRINTH

    def __init__(self, **kwargs):
        mn, mx = np.array([[-12, -12, -12], [12, 12, 12]])
        u0 = np.array([4.6722764, 5.2437205e-10, -6.4444208e-10])
        super().__init__('ThomasLabyrinth', mn, mx, u0, **kwargs)


class FHN_PDE(ODE):
    """2-D FitzHugh-Nagumo on a d_x x d_x periodic grid, d = 2 d_x^2 (systems.py:291-398).
    u0 reproduces the reference's seeded draw (systems.py:303-312: np.random.seed(seed), then a
    Generator over the legacy global bit generator)."""
    kind = _lib.SYS_FHN_PDE

    def __init__(self, d_x, seed=45, **kwargs):
        self.d_x = self.d_y = d_x
        d = 2 * (d_x * d_x)
        self.nx = d_x
        mn, mx = np.array([[-1] * d, [1] * d])
        np.random.seed(seed)
        if hasattr(np.random, 'get_bit_generator'):
            rng = np.random.Generator(np.random.get_bit_generator())
        else:
            rng = np.random.default_rng(seed)
        u0 = rng.uniform(size=d)
        super().__init__(f'FHN_PDE_{d_x}', mn, mx, u0, **kwargs)


class Burgers(ODE):
    """Viscous Burgers on d_x periodic points (systems.py:402-459); nu = param[0]."""
    kind = _lib.SYS_BURGERS

    def __init__(self, d_x, nu=1 / 100, **kwargs):
        self.d_x = d_x
        self.nu = nu
        self.nx = d_x
        mn, mx = np.array([[0] * d_x, [1] * d_x])
        x_fine = np.linspace(-1, 1, num=(d_x - 1) + 1)
        u0 = 0.5 * (np.cos(4.5 * np.pi * x_fine) + 1)
        super().__init__(f'Burgers_{d_x}', mn, mx, u0, param=(float(nu),), **kwargs)


class DiffReact(ODE):
    """2-D diffusion-reaction (FitzHugh-Nagumo reaction, PDEBench) on a d_x x d_x grid with zero-flux
    walls, d = 2 d_x^2, state u | v (systems.py:463-577); param = (Du, Dv, k).  The propagator holds
    one slice per workgroup, so 3 <= d_x <= 32 (larger grids are refused by the library)."""
    kind = _lib.SYS_DIFFREACT

    def __init__(self, d_x: int, Du: float = 1e-3, Dv: float = 5E-3, k: float = 5E-3, seed=45, **kwargs):
        self.d_x = d_x
        self.d_y = d_x
        self.Du = Du
        self.Dv = Dv
        self.k = k
        d = 2 * (d_x * d_x)
        self.nx = d_x
        mn, mx = np.array([[-4] * d, [4] * d])
        u0 = np.random.default_rng(seed).uniform(size=d)
        super().__init__(f'DiffReact2D_{d_x}', mn, mx, u0, param=(float(Du), float(Dv), float(k)), **kwargs)


class _TableODE(ODE):
    """What the table-backed systems (PolyODE, FuncODE) share: the checks of u0, mn and mx, the packing
    of the rows of terms, and the library's table -- made on the first use of the descriptor, destroyed
    with the object.  A subclass sets LABEL (the prefix of its messages) and DESTROY (the library's
    destroy entry point) and has _create(handle_ref), the call of its create entry point."""
    MAX_D, MAX_DEGREE = 2048, 3
    LABEL = DESTROY = None

    @classmethod
    def _state(cls, u0):
        """u0 as a float vector, and d"""
        u0 = np.array(u0, dtype=float)
        if u0.ndim != 1 or not 1 <= u0.shape[0] <= cls.MAX_D:
            raise ValueError(f'{cls.LABEL}: u0 must be a vector of 1..{cls.MAX_D} components')
        return u0, u0.shape[0]

    @classmethod
    def _bounds(cls, terms, d, mn, mx, normalization):
        """mn and mx as the normaliser takes them, after the check of the number of rows"""
        if len(terms) != d:
            raise ValueError(f'{cls.LABEL}: {len(terms)} rows of terms for d = {d}')
        if normalization is not None and normalization.lower() == '-11':
            if mn is None or mx is None:
                raise ValueError(f"{cls.LABEL}: normalization='-11' needs mn and mx")
            mn = np.broadcast_to(np.asarray(mn, dtype=float), (d,)).copy()
            mx = np.broadcast_to(np.asarray(mx, dtype=float), (d,)).copy()
        return mn, mx

    def _pack_terms(self, terms, bound, interval):
        """self.terms and the library's arrays of them; the indices lie in [0, bound), which the
        message calls `interval`"""
        row_ptr, coef, idx = [0], [], []
        for c, row in enumerate(terms):
            for coef_t, ind in row:
                ind = [int(i) for i in ind]
                if len(ind) > self.MAX_DEGREE:
                    raise ValueError(f'{self.LABEL}: row {c} has a term of degree {len(ind)} (at most {self.MAX_DEGREE})')
                if any(not 0 <= i < bound for i in ind):
                    raise ValueError(f'{self.LABEL}: row {c} has an index outside {interval}')
                if not np.isfinite(coef_t):
                    raise ValueError(f'{self.LABEL}: row {c} has a coefficient that is not finite')
                coef.append(float(coef_t))
                idx.append(ind + [-1] * (self.MAX_DEGREE - len(ind)))
            row_ptr.append(len(coef))
        self.terms = [[(float(a), tuple(int(i) for i in ind)) for a, ind in row] for row in terms]
        self._row_ptr = np.array(row_ptr, dtype=np.int32)
        self._coef = np.array(coef, dtype=np.float64)
        self._idx = np.array(idx, dtype=np.int16).reshape(-1, 3)
        self._handle = None

    def _term_args(self):
        """n_terms, row_ptr, coef, idx as the create entry points take them"""
        return (len(self._coef), self._row_ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                self._coef.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                self._idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)))

    @property
    def nx(self):
        """nngp_system.nx of this kind: the table's handle, created on first use"""
        if self._handle is None:
            h = ctypes.c_int32(0)
            _lib.check(self._create(ctypes.byref(h)))
            self._handle = int(h.value)
        return self._handle

    def destroy(self):
        """Free the library's table now (else when the object goes); descriptors made from it are
        refused from then on."""
        h, self._handle = getattr(self, '_handle', None), None
        if h is not None and _lib._lib is not None:
            getattr(_lib._lib, self.DESTROY)(h)   # after nngp_shutdown the table is gone already: ignored

    def __del__(self):
        try:
            self.destroy()
        except Exception:   # interpreter teardown
            pass


class PolyODE(_TableODE):
    """A user-defined polynomial system: the counterpart of subclassing the reference's ODE and
    writing _f_np / _f_jax (systems.py:23-61), with the right-hand side given as data.

    terms[c] is the ordered list of row c's terms (coef, indices), 0 to 3 indices in [0, d) each:
        du_c/dt = sum over the list of  coef * u[i1] * u[i2] * u[i3]
    evaluated exactly as written -- coef times the factors left to right, the first term plus the
    following ones in list order, an empty list giving 0.0.  Brusselator is
        PolyODE([[(1, ()), (1, (0, 0, 1)), (-4, (0,))], [(3, (0,)), (-1, (0, 0, 1))]], u0=[1, 3.07])
    normalization='-11' needs mn and mx.  The library's table (nngp_poly_create) is made on the
    first use of the descriptor and destroyed with the object; everything else is ODE's, so
    SolverRK, Parareal, build_cont_traj and the legacy solver take it like any other system."""
    kind = _lib.SYS_POLY
    MAX_D, MAX_DEGREE = 2048, 3
    LABEL, DESTROY = 'PolyODE', 'nngp_poly_destroy'

    def __init__(self, terms, u0, mn=None, mx=None, name='PolyODE', normalization=None, **kwargs):
        u0, d = self._state(u0)
        mn, mx = self._bounds(terms, d, mn, mx, normalization)
        self._pack_terms(terms, d, f'[0, {d})')
        super().__init__(name, mn, mx, u0, normalization=normalization, **kwargs)

    def _create(self, handle_ref):
        return _lib.lib().nngp_poly_create(self.d, *self._term_args(), handle_ref)


class FuncODE(_TableODE):
    """A user-defined system whose right-hand side is monomials over the state and over
    elementary-function atoms of it: PolyODE with sin, cos, exp, log, 1/x and sqrt.

    atoms[q] is (fn, (a, i)), (fn, (a, i), (c, j)), or either with a trailing scalar b:
        atom_q = fn(a*u[i] + c*u[j] + b),   fn in 'sin', 'cos', 'exp', 'log', 'recip', 'sqrt'
    the argument formed left to right, an absent part not added.  Atoms read the state only.
    terms[c] is PolyODE's ordered list of (coef, indices) for row c, 0 to 3 indices each, where an
    index below d names a state component and d + q names atom q.  A damped pendulum is
        FuncODE(atoms=[('sin', (1.0, 0))], terms=[[(1.0, (1,))], [(-1.0, (2,)), (-0.1, (1,))]], u0=[1.0, 0.0])
    normalization='-11' needs mn and mx; the atoms see the de-normalised state.  The library's table
    (nngp_func_create) is made on the first use of the descriptor and destroyed with the object;
    everything else is ODE's, so SolverRK, SolverScipy, Parareal, build_cont_traj and the legacy
    solver take it like any other system."""
    kind = _lib.SYS_FUNC
    MAX_D, MAX_ATOMS, MAX_DEGREE = 2048, 2048, 3
    FUNCTIONS = _lib.FUNC_FN
    LABEL, DESTROY = 'FuncODE', 'nngp_func_destroy'

    def __init__(self, atoms, terms, u0, mn=None, mx=None, name='FuncODE', normalization=None, **kwargs):
        u0, d = self._state(u0)
        atoms = list(atoms)
        if len(atoms) > self.MAX_ATOMS:
            raise ValueError(f'FuncODE: {len(atoms)} atoms (at most {self.MAX_ATOMS})')
        mn, mx = self._bounds(terms, d, mn, mx, normalization)
        recs, canon = (_lib.CFuncAtom * max(len(atoms), 1))(), []
        for q, atom in enumerate(atoms):
            rec = self._atom(q, atom, d)
            canon.append(rec)
            fn, (a, i), second, b = rec
            c, j = second if second is not None else (0.0, -1)
            recs[q] = _lib.CFuncAtom(self.FUNCTIONS[fn], i, j, int(b is not None), a, c, 0.0 if b is None else b)
        nw = d + len(atoms)
        self._pack_terms(terms, nw, f'[0, d + n_atoms = {nw})')
        self.atoms = canon   # (fn, (a, i), (c, j) or None, b or None)
        self._atoms = recs
        super().__init__(name, mn, mx, u0, normalization=normalization, **kwargs)

    def _create(self, handle_ref):
        return _lib.lib().nngp_func_create(self.d, len(self.atoms), self._atoms, *self._term_args(), handle_ref)

    @classmethod
    def _atom(cls, q, atom, d):
        """atom q as (fn, (a, i), (c, j) or None, b or None), or ValueError"""
        bad = f'FuncODE: atom {q} '
        if not isinstance(atom, (tuple, list)) or not 2 <= len(atom) <= 4:
            raise ValueError(bad + 'must be (fn, (a, i)[, (c, j)][, b])')
        fn, parts = atom[0], list(atom[1:])
        if fn not in cls.FUNCTIONS:
            raise ValueError(bad + f'names the function {fn!r} (one of {", ".join(cls.FUNCTIONS)})')
        b = None
        if np.isscalar(parts[-1]):
            b = float(parts.pop())
            if not np.isfinite(b):
                raise ValueError(bad + 'has an offset b that is not finite')
        if not 1 <= len(parts) <= 2:
            raise ValueError(bad + 'must be (fn, (a, i)[, (c, j)][, b])')
        pairs = []
        for part in parts:
            if not isinstance(part, (tuple, list)) or len(part) != 2:
                raise ValueError(bad + 'has a component that is not a (coefficient, state index) pair')
            a, i = float(part[0]), int(part[1])
            if not np.isfinite(a):
                raise ValueError(bad + 'has a coefficient that is not finite')
            if not 0 <= i < d:
                raise ValueError(bad + f'has a state index outside [0, {d}) (atoms read the state only)')
            pairs.append((a, i))
        return fn, pairs[0], pairs[1] if len(pairs) == 2 else None, b
