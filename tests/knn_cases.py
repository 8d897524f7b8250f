"""Shared inputs of tests/test_knn_cases_host.py (CPU) and tests/test_gpu_knn_matrix.py (GPU): an
independent numpy reference of the kNN select, the input condition of its two algorithms, and the
seeded case tables that put every form of the select (csrc/nngp_gp.hip knn_select_dev), of the
distance row body (knn_dist_row) and of the neighbour geometry after the select at its edges.

The select has five instantiations by ceil(rows/256) -- register keys K = 2, 4, 8, 16 up to
512 / 1024 / 2048 / 4096 rows, streaming K = 0 above, with an LDS key cache up to 14 336 rows --
and each runs the radix threshold select when at most 256 rows have a key whose high word is at or
below the m-th smallest, the m-round fallback otherwise.  No GPU is needed to build a case."""
import functools

import numpy as np

SEL_CAND = 256            # csrc/nngp_gp.hip: candidates the threshold select ranks exactly
KEY_LDS_ROWS = 14336      # rows up to which the streaming select stages its keys in LDS
XS_DOUBLES = 6144         # the select stages the m neighbour rows in LDS while m*(d+1) <= this
NAN_KEY = np.uint64(0x7FF8000000000000)


# ------------------------------------------------------------------------------------ reference
def ref_knn(X, q, m):
    """(idx, s[idx], s): s the column-ordered sequential sum of (q[c] - X[:, c])**2 (elementwise
    the additions of knn_dist_row and of scipy cdist), idx numpy's stable argsort (NaN last)."""
    X = np.asarray(X, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    s = np.zeros(X.shape[0])
    with np.errstate(all='ignore'):
        for c in range(X.shape[1]):
            s = s + (q[c] - X[:, c]) ** 2
    idx = np.argsort(s, kind='stable')[:m]
    return idx.astype(np.int32), s[idx], s


def n_candidates(s, m):
    """Rows the threshold select would have to rank: the key is the distance's bit pattern (one
    key for every NaN), hk its high word, T the m-th smallest hk; the count of hk <= T."""
    s = np.ascontiguousarray(s, dtype=np.float64)
    key = s.view(np.uint64).copy()
    key[np.isnan(s)] = NAN_KEY
    hk = key >> np.uint64(32)
    T = np.sort(hk)[m - 1]
    return int(np.count_nonzero(hk <= T))


# --------------------------------------------------------------------------------- kNN cases
# A case is a dict: id, kind, m, the builder's arguments, `side` (which algorithm its input is
# meant to reach: 'threshold', 'rounds' or None = whatever random data gives) and, for the
# distance-kernel cases, `offset` ('X' / 'q' / None: that array starts one double into its buffer).
EDGE_ROWS = [1, 2, 64, 65, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 14336, 14337]
EDGE_D = [1, 3, 33]
DIST_D = [31, 32, 33, 63, 64, 65, 96, 200]
TIES = [(300, 300, 64), (512, 257, 18), (513, 256, 18), (513, 257, 18), (1024, 257, 64), (2048, 400, 15),
        (4096, 4096, 64), (4096, 257, 1), (5000, 256, 12), (5000, 257, 12), (14337, 300, 18)]
LOWWORD = [(200, 18), (256, 18), (257, 18), (600, 18), (4096, 64), (6000, 20)]


def _cases():
    out = []
    for rows in EDGE_ROWS:
        for d in EDGE_D:
            for m in sorted({1, min(15, rows), min(64, rows)}):
                out.append(dict(id=f'edge-r{rows}-d{d}-m{m}', kind='edge', rows=rows, d=d, m=m, side=None))
    for d in DIST_D:
        for off in (None, 'X', 'q'):
            out.append(dict(id=f'dist-d{d}-{"aligned" if off is None else off + "off"}', kind='edge', rows=300,
                            d=d, m=15, side=None, offset=off))
    for rows, L, m in TIES:
        out.append(dict(id=f'tie-r{rows}-L{L}-m{m}', kind='tie', rows=rows, L=L, m=m,
                        side='threshold' if L <= SEL_CAND else 'rounds'))
    for rows, m in LOWWORD:
        out.append(dict(id=f'low-r{rows}-m{m}', kind='low', rows=rows, m=m,
                        side='threshold' if rows <= SEL_CAND else 'rounds'))
    for m in (1, 5, 64):
        out.append(dict(id=f'nonfinite-r700-m{m}', kind='nonfinite', m=m, side=None))
    out.append(dict(id='nanfill-r100-m30', kind='nanfill', m=30, qinf=False, side='threshold'))
    out.append(dict(id='nanfill-r100-m30-qinf', kind='nanfill', m=30, qinf=True, side='threshold'))
    return out


CASES = _cases()
CASE_IDS = [c['id'] for c in CASES]
TIE_D = 3
NONFINITE_ROWS = dict(nan1=10, nan_all=11, pinf=12, ninf=13, big=14, zero=400, sub160=650, sub155=20)


def case_rows(case):
    return {'nonfinite': 700, 'nanfill': 100}.get(case['kind']) or case['rows']


def build(case):
    """(X [rows][d], q [d]) of a case, C-contiguous float64."""
    kind = case['kind']
    if kind == 'edge':
        rows, d = case['rows'], case['d']
        rng = np.random.default_rng(1000003 * rows + 101 * d + case['m'])
        X = rng.standard_normal((rows, d))
        return X, X[rows // 2] + 1e-3
    if kind == 'tie':
        # L copies of one row at random positions; every other row at distance >= 10 of q = 0
        rows, L = case['rows'], case['L']
        rng = np.random.default_rng(7 * rows + L)
        v = rng.standard_normal((rows, TIE_D))
        X = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(11.0, 20.0, (rows, 1))
        X[tie_positions(case)] = np.array([0.3, -0.2, 0.1])
        return X, np.zeros(TIE_D)
    if kind == 'low':
        # every distance (1 + p * 2**-40)**2 shares one high word and all are distinct
        rows = case['rows']
        p = np.random.default_rng(rows).permutation(rows).astype(np.float64)
        return (1.0 + p * 2.0 ** -40).reshape(rows, 1), np.zeros(1)
    if kind == 'nonfinite':
        R = NONFINITE_ROWS
        X = np.random.default_rng(700).standard_normal((700, 4))
        q = np.zeros(4)
        X[R['nan1'], 2] = np.nan
        X[R['nan_all']] = np.nan
        X[R['pinf'], 0] = np.inf
        X[R['ninf'], 3] = -np.inf
        X[R['big'], 1] = 1e200          # its square overflows
        X[R['zero']] = q                # distance +0
        X[R['sub160']] = q + 1e-160     # subnormal distances (1e-162 would underflow to zero)
        X[R['sub155']] = q + 1e-155
        return X, q
    if kind == 'nanfill':
        # 15 finite rows, one +inf row, the rest NaN: m = 30 runs through +inf into the NaN rows
        rng = np.random.default_rng(100)
        X = np.full((100, 4), np.nan)
        fin = np.sort(rng.choice(100, size=16, replace=False))
        X[fin] = rng.standard_normal((16, 4))
        X[fin[7], 2] = np.inf
        q = 0.1 * rng.standard_normal(4)
        if case['qinf']:   # every finite row at +inf (ties by index), the +inf row at inf - inf = NaN
            q[2] = np.inf
        return X, q
    raise KeyError(kind)


def tie_positions(case):
    """Sorted rows holding the copied row of a tie case."""
    rows, L = case['rows'], case['L']
    return np.sort(np.random.default_rng(rows * 31 + L).choice(rows, size=L, replace=False))


# ------------------------------------------------------------------------- nngp_predict shapes
# (m, d, rows[, copies]); data as in test_predict_every_padded_size_and_fallback_vs_oracle
PREDICT_SHAPES = (
    # padded fit sizes at their edges
    [(1, 3, 40), (2, 3, 40), (8, 3, 40), (9, 3, 40), (25, 4, 90), (32, 3, 100), (49, 3, 150)] +
    # geometry switches: sequential below d = 8, the octet form to d = 128, a wave per pair above
    [(15, 7, 60), (15, 8, 60), (15, 9, 60), (20, 128, 80), (20, 129, 80)] +
    # the staging bound m*(d+1) <= 6144 from both sides
    [(48, 127, 150), (47, 128, 150), (48, 128, 150), (64, 95, 200), (64, 96, 200), (64, 100, 200)] +
    # every select form in front of staged geometry (above 4096 rows the staged keys and the
    # staged rows share the dynamic LDS)
    [(18, 3, 5000), (18, 8, 5000), (18, 3, 14336), (18, 3, 15000), (20, 136, 4500), (18, 3, 600, 300)])


def predict_id(shape):
    return 'm{}-d{}-r{}'.format(*shape[:3]) + (f'-dup{shape[3]}' if len(shape) > 3 else '')


def staged(m, d):
    return m * (d + 1) <= XS_DOUBLES


def geometry_form(m, d, d2_waves=True):
    """Which code computes D2 / kd2 after the select (csrc/nngp_gp.hip d2_by_waves / d2_by_pairs)."""
    if d > 128 or not staged(m, d):
        return 'wave' if d2_waves else 'pairs'
    return 'octet' if d >= 8 else 'sequential'


def predict_data(shape):
    """(X, Y, q) of a predict shape; with `copies`, that many random rows of X become the row q
    sits next to (Y keeps every row's own value: a singular kernel matrix for the fits)."""
    m, d, rows = shape[:3]
    rng = np.random.default_rng(m * 10 + d + rows)
    X = np.cumsum(0.05 * rng.standard_normal((rows, d)), axis=0)
    Y = 0.01 * np.sin(3 * X) + 1e-5 * rng.standard_normal(X.shape)
    q = X[rows // 3] + 0.01
    if len(shape) > 3:
        X[rng.choice(rows, size=shape[3], replace=False)] = X[rows // 3]
    return X, Y, q


def draw_thetas(d, n_predictions, seed):
    """NNGP_p.draw_thetas (models.py:192): the stream a model seeded `seed` draws first."""
    import nngp_amd
    return nngp_amd.NNGP_p(n=d, N=4, nn=10, seed=seed).draw_thetas(n_predictions)


# ------------------------------------------------------------------------------- sweep cases
SWEEP_N, SWEEP_M, SWEEP_NG, SWEEP_NF = 8, 18, 2, 40
# (rows, copies of one training row near traj[2], seed)
SWEEP_CASES = {'r5000': (5000, 0, 5), 'r15000': (15000, 0, 5), 'r600dup': (600, 300, 5)}


@functools.lru_cache(maxsize=None)
def sweep_case(name, m=SWEEP_M):
    """A synthetic correction sweep on Lorenz '-11' (N = 8, I = 0, G = RK1 with 2 steps, m = 18
    unless given) and the oracle's loop over it, all on the CPU.  The training set is rows//8 points
    per slice around the fine trajectory with Y = F - G there; UF / UG are the "previous iteration" whose
    guess chain (nngp_sweep.hip: g[0] = U1[0], g[i+1] = G(g[i]) + (UF[i+1] - UG[i+1])) leaves the
    actual chain at slice 5.  Returns a dict of host arrays and the predicted hit of every slice."""
    import oracle as O
    D = _sweep_data(name)
    t, traj, X, Y, UF, UG, th0, per = (D[k] for k in ('t', 'traj', 'X', 'Y', 'UF', 'UG', 'th0', 'per'))
    N = SWEEP_N
    so = O.System('lorenz')
    G = lambda i, u: so.rk(1, t[i], t[i + 1], SWEEP_NG, u)
    nf = th0.shape[0] // N
    U1 = np.zeros((N + 1, 3))
    UG1 = np.zeros((N + 1, 3))
    U1[0] = traj[0]
    g = np.zeros((N, 3))
    g[0] = U1[0]
    for i in range(N):
        UG1[i + 1] = G(i, U1[i])
        U1[i + 1] = O.predict(X, Y, U1[i], m, th0[i * nf:(i + 1) * nf]) + UG1[i + 1]
        if i + 1 < N:
            g[i + 1] = G(i, g[i]) + (UF[i + 1] - UG[i + 1])
    hit = [bool(np.array_equal(O.knn(X, g[i], m)[0], O.knn(X, U1[i], m)[0])) for i in range(N)]
    ncand_q = [n_candidates(ref_knn(X, U1[i], m)[2], m) for i in range(N)]
    ncand_g = [n_candidates(ref_knn(X, g[i], m)[2], m) for i in range(N)]
    return dict(t=t, traj=traj, X=X, Y=Y, UF=UF, UG=UG, th0=th0, U1=U1, UG1=UG1, g=g, hit=hit,
                ncand_q=ncand_q, ncand_g=ncand_g, rows=per * N, m=m, N=N)


@functools.lru_cache(maxsize=None)
def _sweep_data(name):
    """The part of a sweep case that does not depend on m: training set, previous iteration, draws."""
    import oracle as O
    rows, copies, seed = SWEEP_CASES[name]
    N = SWEEP_N
    so = O.System('lorenz')
    t = np.linspace(0, 0.4, N + 1)
    F = lambda i, u: so.rk(4, t[i], t[i + 1], SWEEP_NF, u)
    G = lambda i, u: so.rk(1, t[i], t[i + 1], SWEEP_NG, u)
    rng = np.random.default_rng(seed)
    traj = np.empty((N + 1, 3))
    traj[0] = [0.1, 0.2, -0.3]
    for i in range(N):
        traj[i + 1] = F(i, traj[i])
    per = rows // N
    X = np.empty((per * N, 3))
    Y = np.empty_like(X)
    for i in range(N):
        X[i * per:(i + 1) * per] = traj[i] + 0.02 * rng.standard_normal((per, 3))
    for r in range(per * N):
        i = r // per
        Y[r] = F(i, X[r]) - G(i, X[r])
    if copies:   # one training row near traj[2], `copies` times (Y keeps every row's own value)
        src = 2 * per + int(np.argmin(np.sum((X[2 * per:3 * per] - traj[2]) ** 2, axis=1)))
        X[rng.choice(per * N, size=copies, replace=False)] = X[src]
    UF = np.zeros((N + 1, 3))
    UG = np.zeros((N + 1, 3))
    for i in range(N):
        u = traj[i] + 1e-6 * rng.standard_normal(3)
        UF[i + 1] = F(i, u)
        UG[i + 1] = G(i, u)
    UF[5] += 0.03
    th0 = draw_thetas(3, N, seed=45)
    return dict(t=t, traj=traj, X=X, Y=Y, UF=UF, UG=UG, th0=th0, per=per)
