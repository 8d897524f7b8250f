"""NumPy restatement of the arithmetic contract of FuncODE (include/nngp.h,
nngp_func_create): the normative text of the kind and the bitwise yardstick of
tests/test_gpu_func.py, itself checked on the CPU by tests/test_func_host.py.  Not a test module.

A system is d state components, n_atoms >= 0 atoms and d rows of terms.

Atom q is (fn, (a, i)[, (c, j)][, b]), i and j state indices in [0, d).  Its argument is formed in
this order, one rounding per operation:
    x = a * u[i];   if a second component is present: x = x + c * u[j];   if b is present: x = x + b
An absent part is not replaced by + 0.0 (that would change the sign of a zero).  Its value is fn(x):
    1 sin    the project's nn_sin_pi (the sine ThomasLabyrinth uses)   oracle orc_sin_pi_array
    2 cos    nn_cos                                                    oracle orc_sincos_array
    3 exp    nn_exp                                                    oracle orc_exp_array
    4 log    nn_log                                                    oracle orc_log_array
    5 recip  IEEE 1.0 / x                                              NumPy 1.0 / x
    6 sqrt   IEEE sqrt(x)                                              NumPy sqrt
Atoms read the state only.  A domain error gives what the routine gives (NaN, inf).

Terms are PolyODE's (tests/poly_ref.py) over w = [u_0 .. u_{d-1}, atom_0 .. atom_{n_atoms-1}]: row c
is an ordered list of (coef, (i1 .. ip)), 0 <= p <= 3, indices in [0, d + n_atoms); a term is coef
times the factors left to right; a row is its first term, then acc + term in list order; a row
without terms is +0.0 (the sum does not start from 0.0).

The '-11' wrapper, the stage input, the step update and both step modes are the existing ones
(poly_ref.rk_np, adaptive_ref.solve); with '-11' the atoms see the de-normalised state.  The exact
build uses no fma beyond those inside the nn_* routines."""
import ctypes

import numpy as np

from poly_ref import PolyNP

FN = {'sin': 1, 'cos': 2, 'exp': 3, 'log': 4, 'recip': 5, 'sqrt': 6}
_DP = ctypes.POINTER(ctypes.c_double)


def _oracle_map(name, x):
    """the oracle's array routine `name` on x (any shape)"""
    import oracle as O
    L = O.lib()
    a = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(a)
    if name == 'orc_sincos_array':   # (n, x, sin, cos): the cosine
        sn = np.empty_like(a)
        L.orc_sincos_array(a.size, a.ctypes.data_as(_DP), sn.ctypes.data_as(_DP), out.ctypes.data_as(_DP))
    else:
        getattr(L, name)(a.size, a.ctypes.data_as(_DP), out.ctypes.data_as(_DP))
    return out


def apply_fn(fn, x):
    x = np.asarray(x, dtype=np.float64)
    if fn == 'sin':
        return _oracle_map('orc_sin_pi_array', x)
    if fn == 'cos':
        return _oracle_map('orc_sincos_array', x)
    if fn == 'exp':
        return _oracle_map('orc_exp_array', x)
    if fn == 'log':
        return _oracle_map('orc_log_array', x)
    with np.errstate(all='ignore'):
        if fn == 'recip':
            return 1.0 / x
        if fn == 'sqrt':
            return np.sqrt(x)
    raise ValueError(fn)


def parse_atom(atom):
    """(fn, (a, i), (c, j) or None, b or None) of the user's tuple"""
    fn, parts = atom[0], list(atom[1:])
    b = float(parts.pop()) if np.isscalar(parts[-1]) else None
    first = (float(parts[0][0]), int(parts[0][1]))
    second = (float(parts[1][0]), int(parts[1][1])) if len(parts) == 2 else None
    return fn, first, second, b


class FuncNP:
    """f_n(u) of a system with atoms, batched over the leading axes; optionally inside the '-11'
    wrapper on [mn, mx] as the kernels form it ((u+1)*((mx-mn)/2) + mn, f * (2/(mx-mn)))."""

    def __init__(self, atoms, rows, mn=None, mx=None):
        self.atoms = [parse_atom(a) for a in atoms]
        self.rows = rows
        self.d = d = len(rows)
        self.n_atoms = len(self.atoms)
        assert all(0 <= a[1][1] < d and (a[2] is None or 0 <= a[2][1] < d) for a in self.atoms)
        self.normalized = mn is not None
        if self.normalized:
            mn = np.broadcast_to(np.asarray(mn, dtype=np.float64), (d,))
            mx = np.broadcast_to(np.asarray(mx, dtype=np.float64), (d,))
            self.mn, self.hw, self.sc = mn, 0.5 * (mx - mn), 2 / (mx - mn)
        # the term walk is PolyNP's, over d + n_atoms columns; only the first d rows exist
        self._poly = PolyNP(list(rows) + [[] for _ in range(self.n_atoms)])
        # atoms grouped by (function, shape of the argument): the same operations per atom
        self.groups = {}
        for q, (fn, _, second, b) in enumerate(self.atoms):
            self.groups.setdefault((fn, second is not None, b is not None), []).append(q)

    def atom_values(self, U):
        """[..., n_atoms] from the (de-normalised) state [..., d]"""
        U = np.asarray(U, dtype=np.float64)
        out = np.empty(U.shape[:-1] + (self.n_atoms,))
        for (fn, has2, hasb), qs in self.groups.items():
            a = np.array([self.atoms[q][1][0] for q in qs])
            i = np.array([self.atoms[q][1][1] for q in qs])
            x = a * U[..., i]
            if has2:
                c = np.array([self.atoms[q][2][0] for q in qs])
                j = np.array([self.atoms[q][2][1] for q in qs])
                x = x + c * U[..., j]
            if hasb:
                x = x + np.array([self.atoms[q][3] for q in qs])
            out[..., qs] = apply_fn(fn, x)
        return out

    def raw(self, U):
        U = np.asarray(U, dtype=np.float64)
        W = np.concatenate([U, self.atom_values(U)], axis=-1) if self.n_atoms else U
        return self._poly.raw(W)[..., :self.d]

    def __call__(self, U):
        if not self.normalized:
            return self.raw(U)
        return self.raw((np.asarray(U, dtype=np.float64) + 1) * self.hw + self.mn) * self.sc

    def term_magnitudes(self, U):
        """sum over each row's terms of |term| at the de-normalised state U: the scale of the
        fixture bound (16 + n_terms) eps sum|term|, per row"""
        U = np.asarray(U, dtype=np.float64)
        W = np.concatenate([U, self.atom_values(U)], axis=-1) if self.n_atoms else U
        out = np.zeros(U.shape[:-1] + (self.d,))
        for c, row in enumerate(self.rows):
            for coef, ind in row:
                v = np.full(U.shape[:-1], abs(coef))
                for i in ind:
                    v = v * np.abs(W[..., i])
                out[..., c] += v
        return out


# ------------------------------------------------------------------------------------------------
# the systems of the tests: name -> dict(atoms, rows, u0, mn, mx, spread, dt[, tscale])
#   u0: the initial condition and the centre of the test inputs (physical units); spread: their
#   half-width; dt: the step of the fixture's 32-step runs; tscale: a factor on the spans of the
#   kernel-form tests (a stiff system needs short explicit steps)
# ------------------------------------------------------------------------------------------------
THOMAS_ATOMS = [('sin', (1.0, 1)), ('sin', (1.0, 2)), ('sin', (1.0, 0))]
THOMAS_ROWS = [[(-0.5, (0,)), (10.0, (3,))], [(-0.5, (1,)), (10.0, (4,))], [(-0.5, (2,)), (10.0, (5,))]]
THOMAS_U0 = [4.6722764, 5.2437205e-10, -6.4444208e-10]
THOMAS_BOUNDS = ([-12.0] * 3, [12.0] * 3)


def pendulum():
    """theta' = omega, omega' = -sin(theta) - 0.1 omega"""
    return dict(atoms=[('sin', (1.0, 0))], rows=[[(1.0, (1,))], [(-1.0, (2,)), (-0.1, (1,))]],
                u0=[1.0, 0.0], mn=[-2.0, -2.0], mx=[2.0, 2.0], spread=0.3, dt=0.05)


def pendulum_cos():
    """the pendulum measured from the horizontal: omega' = -cos(theta - 1.25) - 0.1 omega"""
    return dict(atoms=[('cos', (1.0, 0), -1.25)], rows=[[(1.0, (1,))], [(-1.0, (2,)), (-0.1, (1,))]],
                u0=[1.0, 0.0], mn=[-2.0, -2.0], mx=[2.0, 2.0], spread=0.3, dt=0.05)


CHEMO = dict(D=0.3, s0=2.0, mu=1.2, K=0.5, Y=0.6)


def chemostat():
    """s' = D (s0 - s) - mu s x / (K + s),  x' = Y mu s x / (K + s) - D x"""
    p = CHEMO
    return dict(atoms=[('recip', (1.0, 0), p['K'])],
                rows=[[(p['D'] * p['s0'], ()), (-p['D'], (0,)), (-p['mu'], (0, 1, 2))],
                      [(p['Y'] * p['mu'], (0, 1, 2)), (-p['D'], (1,))]],
                u0=[1.0, 0.5], mn=[0.0, 0.0], mx=[3.0, 2.0], spread=0.2, dt=0.05)


GOMP = dict(r=0.8, invK=0.5, q=0.5, k=0.4)


def gompertz_tanks():
    """x' = -r x log(x / K);  a two-tank cascade h1' = q - k sqrt(h1), h2' = k sqrt(h1) - k sqrt(h2)"""
    p = GOMP
    return dict(atoms=[('log', (p['invK'], 0)), ('sqrt', (1.0, 1)), ('sqrt', (1.0, 2))],
                rows=[[(-p['r'], (0, 3))], [(p['q'], ()), (-p['k'], (4,))], [(p['k'], (4,)), (-p['k'], (5,))]],
                u0=[0.5, 1.0, 0.6], mn=[0.1, 0.1, 0.1], mx=[3.0, 3.0, 3.0], spread=0.2, dt=0.05)


KURA_N, KURA_K = 8, 1.5


def kuramoto_omega():
    return 1.0 + 0.25 * np.cos(1.0 + 1.7 * np.arange(KURA_N))


def kuramoto():
    """theta_i' = omega_i + (K/N) sum_{j != i} sin(theta_j - theta_i): 56 atoms, j ascending"""
    n, om = KURA_N, kuramoto_omega()
    atoms, rows = [], []
    for i in range(n):
        row = [(float(om[i]), ())]
        for j in range(n):
            if j != i:
                row.append((KURA_K / n, (n + len(atoms),)))
                atoms.append(('sin', (1.0, j), (-1.0, i)))
        rows.append(row)
    u0 = 0.4 * np.arange(n) - 1.0
    return dict(atoms=atoms, rows=rows, u0=list(u0), mn=[-4.0] * n, mx=[8.0] * n, spread=0.3, dt=0.05)


SG_POINTS = 32


def sine_gordon(points=SG_POINTS, length=16.0):
    """u_tt = u_xx - sin u on a periodic line of `points` points by the method of lines: the state is
    u | v, d = 2 points; u_i' = v_i, v_i' = c u_{i-1} + (-2c) u_i + c u_{i+1} - sin u_i"""
    n = points
    c = 1.0 / (length / n) ** 2
    atoms = [('sin', (1.0, i)) for i in range(n)]
    rows = [[(1.0, (n + i,))] for i in range(n)]
    rows += [[(c, ((i - 1) % n,)), (-2.0 * c, (i,)), (c, ((i + 1) % n,)), (-1.0, (2 * n + i,))] for i in range(n)]
    x = length * np.arange(n) / n
    u0 = np.concatenate([4.0 * np.arctan(np.exp(-0.5 * (x - length / 2) ** 2 + 1.0)), 0.2 * np.sin(2 * np.pi * x / length)])
    return dict(atoms=atoms, rows=rows, u0=list(u0), mn=[-8.0] * (2 * n), mx=[8.0] * (2 * n), spread=0.2, dt=0.02)


BRATU_D, BRATU_LAM = 40, 2.0


def bratu(d=BRATU_D, lam=BRATU_LAM):
    """u_t = u_xx + lambda exp(u) on (0, 1), u = 0 at both ends, d inner points"""
    c = float((d + 1) ** 2)
    atoms = [('exp', (1.0, i)) for i in range(d)]
    rows = []
    for i in range(d):
        row = []
        if i > 0:
            row.append((c, (i - 1,)))
        row.append((-2.0 * c, (i,)))
        if i + 1 < d:
            row.append((c, (i + 1,)))
        row.append((lam, (d + i,)))
        rows.append(row)
    x = np.arange(1, d + 1) / (d + 1)
    u0 = 0.3 * np.sin(np.pi * x) + 0.05
    return dict(atoms=atoms, rows=rows, u0=list(u0), mn=[-1.0] * d, mx=[2.0] * d, spread=0.04, dt=1e-4, tscale=0.01)


GOLDEN_SYSTEMS = {'pendulum': pendulum, 'pendulum_cos': pendulum_cos, 'chemostat': chemostat, 'gompertz': gompertz_tanks, 'kuramoto': kuramoto,
                  'sinegordon': sine_gordon, 'bratu': bratu}
# classic Parareal of the fixture, '-11', F = RK4, eps 5e-7: (T, N, Ng, Nf, G)
GOLDEN_PARA = {'pendulum': (8.0, 8, 20, 80, 'RK1'), 'sinegordon': (4.0, 8, 8, 80, 'RK2')}


def n_terms(rows):
    return sum(len(r) for r in rows)


def golden_states(name, n, seed, norm):
    """n test inputs around the system's u0 (physical units, or their '-11' images when norm)"""
    S = GOLDEN_SYSTEMS[name]()
    rng = np.random.default_rng(seed)
    U = np.array(S['u0']) + S['spread'] * rng.uniform(-1, 1, (n, len(S['u0'])))
    if norm:
        mn, mx = np.asarray(S['mn']), np.asarray(S['mx'])
        U = 2 * (U - mn) / (mx - mn) - 1
    assert not np.any(U == 0.0)
    return U


def synthetic(d, n_atoms, seed=0, rows_terms=3, shift=0):
    """A system of any shape for the kernel-form tests: atom q cycles through all six functions (from
    function `shift` on) and all four argument shapes, each with an argument range its function is at home in for states in
    [1, 2]^d; row c is a constant, a linear term, and `rows_terms - 2` terms that each name an atom
    (n_atoms > 0) or two more state components.  Bounded right-hand sides: short runs stay in [0.5, 2.5]^d."""
    rng = np.random.default_rng(1000 * d + n_atoms + seed)
    fns = ['sin', 'cos', 'exp', 'log', 'recip', 'sqrt']
    atoms = []
    for q in range(n_atoms):
        fn = fns[(q + shift) % 6]
        i, j = int(rng.integers(d)), int(rng.integers(d))
        a, c, b = float(rng.uniform(0.5, 1.5)), float(rng.uniform(0.25, 0.75)), float(rng.uniform(0.25, 1.0))
        if fn == 'exp':   # exp(2.6) at most
            a, c = 0.4 * a, 0.4 * c
        shape = (q + q // 6) % 4
        atoms.append([(fn, (a, i)), (fn, (a, i), (c, j)), (fn, (a, i), b), (fn, (a, i), (c, j), b)][shape])
    rows = []
    counts = [rows_terms] * d if np.isscalar(rows_terms) else list(rows_terms)   # terms per row (>= 2)
    for c in range(d):
        row = [(float(rng.uniform(-0.2, 0.2)), ()), (float(rng.uniform(-0.5, -0.1)), (c,))]
        for _ in range(counts[c] - 2):
            coef = float(rng.uniform(-0.3, 0.3))
            if n_atoms:
                q = int(rng.integers(n_atoms))
                ind = (d + q,) if rng.integers(2) else (int(rng.integers(d)), d + q)
            else:
                ind = (int(rng.integers(d)), int(rng.integers(d)))
            row.append((coef, ind))
        rows.append(row)
    return dict(atoms=atoms, rows=rows, u0=[1.5] * d, mn=[0.25] * d, mx=[3.0] * d, spread=0.4)


def synthetic_states(S, n, seed, norm):
    rng = np.random.default_rng(seed)
    d = len(S['u0'])
    U = np.array(S['u0']) + S['spread'] * rng.uniform(-1, 1, (n, d))
    if norm:
        mn, mx = np.asarray(S['mn']), np.asarray(S['mx'])
        U = 2 * (U - mn) / (mx - mn) - 1
    assert not np.any(U == 0.0)
    return U
