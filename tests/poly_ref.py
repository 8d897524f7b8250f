"""NumPy restatement of the polynomial field's arithmetic contract and of the RK
step in the operation order of csrc/nngp_rk_dev.h (stage_input / step_update / LinGrid), with all
four tableaux transcribed from csrc/tableau.h: the bitwise yardstick of tests/test_gpu_poly.py,
itself checked on the CPU by tests/test_poly_host.py.  NumPy's elementwise fp64 add and mul are
IEEE, one rounding per operation, so this is bit-reproducible.  Everything is batched over the
leading axis (one row per slice), which changes no element's operations.  Not a test module."""
import numpy as np

_h = float.fromhex
_Z = 0.0
# csrc/tableau.h; zero entries are skipped, as in the kernels
TABLEAUX = {
    1: ([[0.0]], [1.0]),
    2: ([[0.0, 0.0], [0.5, 0.0]], [0.0, 1.0]),
    4: ([[0.0, 0.0, 0.0, 0.0], [0.5, 0.0, 0.0, 0.0], [0.0, 0.5, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]],
        [1.0 / 6, 1.0 / 3, 1.0 / 3, 1.0 / 6]),
    8: ([[_Z] * 11,
         [_h('0x1.0000000000000p-1')] + [_Z] * 10,
         [_h('0x1.0000000000000p-2'), _h('0x1.0000000000000p-2')] + [_Z] * 9,
         [_h('0x1.2492492492492p-3'), _h('-0x1.b195cca340900p-3'), _h('0x1.cad842e9913b0p-1')] + [_Z] * 8,
         [_h('0x1.7beb04681f33ep-3'), _Z, _h('0x1.27417bb787106p-1'), _h('0x1.0ad929c2b65f7p-4')] + [_Z] * 7,
         [_h('0x1.98db47b6369adp-3'), _Z, _h('0x1.82594c40962e5p-2'), _h('-0x1.da940cb6a5369p-2'),
          _h('0x1.8bcd1c9af3badp-2')] + [_Z] * 6,
         [_h('0x1.0829f72fc1982p-3'), _Z, _h('-0x1.0e8b8460f0c4bp-5'), _h('-0x1.6619247fe45f5p-2'),
          _h('0x1.5066d0fa779f1p-2'), _h('0x1.910011977ae2cp-4')] + [_Z] * 5,
         [_h('0x1.2492492492492p-4'), _Z, _Z, _Z, _h('0x1.066d8aec55c72p-9'), _h('-0x1.84e9bc91f59e8p-7'),
          _h('0x1.c71c71c71c71cp-4')] + [_Z] * 4,
         [_h('0x1.0000000000000p-5'), _Z, _Z, _Z, _h('-0x1.29c2f45fc00d5p-7'), _h('0x1.38e38e38e38e4p-3'),
          _h('-0x1.43dd1722cc702p-1'), _h('0x1.ea4b3f66128ccp-1')] + [_Z] * 3,
         [_h('0x1.2492492492492p-4'), _Z, _Z, _Z, _h('0x1.c71c71c71c71cp-4'), _h('-0x1.469ef01c47156p-1'),
          _h('0x1.03fa884516df4p+1'), _h('-0x1.cf94b916c05b2p+0'), _h('0x1.0fffe5f0ee105p+0')] + [_Z] * 2,
         [_Z, _Z, _Z, _Z, _h('-0x1.1a3994e68f664p-1'), _h('0x1.39c6d581a481cp+1'), _h('-0x1.ca8e90f5a3677p+2'),
          _h('0x1.e3721f2e86f5bp+2'), _h('-0x1.1d550e6532babp+1'), _h('0x1.e15606adabd80p-1'), _Z]],
        [_h('0x1.999999999999ap-5'), _Z, _Z, _Z, _Z, _Z, _Z, _h('0x1.16c16c16c16c1p-2'),
         _h('0x1.6c16c16c16c17p-2'), _h('0x1.16c16c16c16c1p-2'), _h('0x1.999999999999ap-5')]),
}


def rk_np(f, order, t0, t1, steps, u0, mode='fixed', gsteps=None, j0=0):
    """`steps` steps of tableau `order`.  u0 [d] with scalar t0, t1, or u0 [n][d] with t0, t1 [n]
    (f then maps [n][d] to [n][d]).  mode 'fixed': h = (t1-t0)/steps; 'linspace': h_n = t[n+1]-t[n]
    on t[j] = j*dt + t0, t[steps] = t1 (LinGrid).  With gsteps: steps j0 .. j0+steps-1 of the grid of
    gsteps steps over [t0, t1] (nngp_rk_batch_grid; a prefix of a trajectory), in fixed mode `steps`
    steps of h = (t1-t0)/gsteps."""
    A, B = TABLEAUX[order]
    S = len(B)
    u = np.array(u0, dtype=np.float64)
    t0 = np.asarray(t0, dtype=np.float64)
    t1 = np.asarray(t1, dtype=np.float64)
    if u.ndim == 2:
        t0, t1 = t0.reshape(-1, 1), t1.reshape(-1, 1)
    if gsteps is None:
        gsteps = steps
    dt = (t1 - t0) / np.float64(gsteps)
    jd = np.float64(j0)
    tn = jd * dt + t0
    for n in range(steps):
        if mode == 'linspace':
            jd = jd + np.float64(1.0)
            tn1 = t1 if n == gsteps - 1 - j0 else jd * dt + t0
            h = tn1 - tn
            tn = tn1
        else:
            h = dt
        k = []
        for s in range(S):
            t = None
            for j in range(s):
                if A[s][j] != 0.0:
                    v = A[s][j] * k[j]
                    t = v if t is None else t + v
            x = u if t is None else u + t
            k.append(h * f(x))
        acc = None
        for s in range(S):
            if B[s] != 0.0:
                v = B[s] * k[s]
                acc = v if acc is None else acc + v
        u = u + acc
    return u


class PolyNP:
    """f_n(u) of a polynomial system: rows[c] = [(coef, (i1, ...)), ...], optionally inside the
    '-11' wrapper on [mn, mx] as the kernels form it ((u+1)*((mx-mn)/2) + mn, f * (2/(mx-mn))).

    The contract: a term is coef, then times u[i1], u[i2], u[i3] left to right; a row is its first
    term, then acc + term in list order; a row without terms is +0.0."""

    def __init__(self, rows, mn=None, mx=None):
        self.rows = rows
        self.d = d = len(rows)
        self.normalized = mn is not None
        if self.normalized:
            mn = np.broadcast_to(np.asarray(mn, dtype=np.float64), (d,))
            mx = np.broadcast_to(np.asarray(mx, dtype=np.float64), (d,))
            self.mn, self.hw, self.sc = mn, 0.5 * (mx - mn), 2 / (mx - mn)
        # position q of every row that has one: (rows, coef, idx [n][3] with -1 = no factor)
        self.levels = []
        q = 0
        while True:
            rs = [c for c in range(d) if len(rows[c]) > q]
            if not rs:
                break
            coef = np.array([rows[c][q][0] for c in rs], dtype=np.float64)
            idx = np.array([list(rows[c][q][1]) + [-1] * (3 - len(rows[c][q][1])) for c in rs], dtype=np.int64)
            assert idx.shape == (len(rs), 3) and np.all(idx < d)
            self.levels.append((np.array(rs), coef, idx))
            q += 1

    def raw(self, U):
        U = np.asarray(U, dtype=np.float64)
        out = np.zeros(U.shape)   # a row without terms: +0.0
        for q, (rs, coef, idx) in enumerate(self.levels):
            v = np.broadcast_to(coef, U.shape[:-1] + coef.shape).copy()
            for s in range(3):
                m = idx[:, s] >= 0
                v[..., m] = v[..., m] * U[..., idx[m, s]]
            out[..., rs] = v if q == 0 else out[..., rs] + v
        return out

    def __call__(self, U):
        if not self.normalized:
            return self.raw(U)
        return self.raw((np.asarray(U, dtype=np.float64) + 1) * self.hw + self.mn) * self.sc


# ------------------------------------------------------------------------------------------------
# the systems of the tests: rows, a state to scatter the inputs around, '-11' bounds
# ------------------------------------------------------------------------------------------------
BRUS = [[(1.0, ()), (1.0, (0, 0, 1)), (-4.0, (0,))], [(3.0, (0,)), (-1.0, (0, 0, 1))]]
LORENZ = [[(10.0, (1,)), (-10.0, (0,))], [(28.0, (0,)), (-1.0, (1,)), (-1.0, (0, 2))],
          [(1.0, (0, 1)), (-(8.0 / 3), (2,))]]
LOGISTIC = [[(1.5, (0,)), (-0.5, (0, 0))]]
_MU = 1.0 / 7
# the Hopf normal form with time as the third component, as the project's Hopf: 9 terms
HOPF_NF = [[(-1.0, (1,)), (_MU, (0, 2)), (-1.0, (0, 0, 0)), (-1.0, (0, 1, 1))],
           [(1.0, (0,)), (_MU, (1, 2)), (-1.0, (0, 0, 1)), (-1.0, (1, 1, 1))],
           [(1.0, ())]]
# d = 4 with exactly 16 terms (rows of 6, 1, 5 and 4): the lane form's cap; and one term more
D4_16 = [[(0.3, ()), (-1.1, (0,)), (0.7, (1, 2)), (-0.2, (3, 3, 0)), (0.5, (2,)), (-0.9, (0, 1, 3))],
         [(-0.6, (1, 1))],
         [(1.3, (3,)), (-0.4, (2, 2, 2)), (0.8, (0, 3)), (-1.7, ()), (0.1, (1,))],
         [(0.9, (0,)), (-0.5, (3,)), (0.2, (1, 2, 3)), (-0.3, (2, 0))]]
D4_17 = [list(r) for r in D4_16]
D4_17[3] = D4_17[3] + [(0.6, (1, 1, 0))]
# a row without terms and a row that is one constant
SPARSE = [[], [(0.7, ())], [(-0.3, (2,)), (0.5, (0, 1))]]


def lorenz96(d, forcing=8.0):
    """du_i = (u_{i+1} - u_{i-2}) u_{i-1} - u_i + F as four monomials per row"""
    return [[(1.0, ((i + 1) % d, (i - 1) % d)), (-1.0, ((i - 2) % d, (i - 1) % d)), (-1.0, (i,)), (forcing, ())]
            for i in range(d)]


VDP = [[(1.0, (1,))], [(1.0, (1,)), (-1.0, (0, 0, 1)), (-1.0, (0,))]]   # Van der Pol, mu = 1


def n_terms(rows):
    return sum(len(r) for r in rows)


# name: (rows, centre of the test inputs, their spread, (mn, mx) of the '-11' runs)
SMALL = {
    'logistic': (LOGISTIC, [0.4], 0.2, ([-1.0], [4.0])),
    'brus': (BRUS, [1.0, 3.07], 0.3, ([0.4, 0.9], [4.0, 5.0])),
    'lorenz': (LORENZ, [-15.0, -15.0, 20.0], 1.0, ([-17.1, -23.0, 6.0], [18.1, 25.0, 45.0])),
    'hopf_nf': (HOPF_NF, [0.4, -0.3, 2.0], 0.2, ([-3.0, -3.0, 0.0], [3.0, 3.0, 9.0])),
    'd4_16': (D4_16, [0.5, -0.4, 0.3, 0.6], 0.2, ([-2.0] * 4, [2.5] * 4)),
    'd4_17': (D4_17, [0.5, -0.4, 0.3, 0.6], 0.2, ([-2.0] * 4, [2.5] * 4)),
    'sparse': (SPARSE, [0.5, -0.4, 0.3], 0.2, ([-2.0] * 3, [2.5] * 3)),
}
assert n_terms(HOPF_NF) == 9 and n_terms(D4_16) == 16 and n_terms(D4_17) == 17
L96_BOUNDS = (-12.0, 16.0)


def states(name_or_d, n, seed, norm):
    """n input states without an exact zero (the contract leaves the sign of a zero sum open): in
    physical units around the system's centre, or their '-11' images when norm"""
    rng = np.random.default_rng(seed)
    if isinstance(name_or_d, str):
        _, centre, spread, (mn, mx) = SMALL[name_or_d]
        U = np.array(centre) + spread * rng.uniform(-1, 1, (n, len(centre)))
    else:
        U = 2.0 + 3.0 * rng.uniform(-1, 1, (n, name_or_d))
        mn, mx = L96_BOUNDS
    if norm:
        mn, mx = np.asarray(mn, dtype=float), np.asarray(mx, dtype=float)
        U = 2 * (U - mn) / (mx - mn) - 1
    assert not np.any(U == 0.0)
    return U


def spans(n):
    """another t0 / t1 for every slice"""
    T0 = 0.25 + 0.0625 * np.arange(n)
    return T0, T0 + 0.02 + 0.0005 * np.arange(n)
